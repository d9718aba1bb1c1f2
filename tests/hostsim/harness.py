"""Test harness: runs the C ABI of the kernel sources built against the host-side HIP simulator.

TEST INFRASTRUCTURE ONLY - the product package never loads this library.
"""
import ctypes as C
import os
import subprocess

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "build", "libdiffmst_hostsim.so")


def build():
    subprocess.run(["make", "-s", "-j8", "-C", HERE], check=True)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        from mst import _cabi

        build()
        _lib = _cabi.bind(C.CDLL(LIB))
    return _lib


def _workspace(nbytes, fill):
    """fp32 workspace of `nbytes` bytes filled with `fill`, starting on a 256-byte boundary like a device allocation."""
    ws = torch.full((nbytes // 4 + 64,), fill)
    return ws[(-ws.data_ptr() % 256) // 4:]


def _nan(*shape):
    return torch.full(shape, float("nan"))


def console(param_ranges, tracks, tp, fp, mp, flags, grad_mix=None, want_mixed=True, grad_mixed=None,
            want_grad_tracks=False, sample_rate=44100, multipass_eq=False, denormalized=False, fx_noise=None,
            fx_ir_samples=65536, fx_bandpass_taps=1023):
    """CPU tensors in; returns dict(mix, mixed, status, grad_tp, grad_mp, grad_tracks)."""
    from mst import _cabi, _desc

    L = lib()
    bs, T, n = tracks.shape
    tracks = tracks.contiguous().float()
    word = _desc.flag_word(save_for_backward=grad_mix is not None, **flags)
    if multipass_eq:
        word |= _cabi.DEV_MULTIPASS_EQ
    if denormalized:  # tp / mp hold denormalised values (forward_mix_console): identity ranges, no range check
        word |= _cabi.NO_RANGE_CHECK
    d = _desc.make_desc(param_ranges, sample_rate, bs, T, n, tracks.stride(1), word, identity_ranges=denormalized,
                        fx_ir_samples=fx_ir_samples, fx_bandpass_taps=fx_bandpass_taps)
    nbytes = L.mst_console_workspace_bytes(d)
    assert nbytes > 0
    ws = _workspace(nbytes, 0.0)
    mix = torch.zeros(bs, 2, n)
    mixed = torch.zeros(bs, 2, T, n) if want_mixed else None
    status = torch.zeros(1, dtype=torch.int32)
    tp, fp, mp = tp.contiguous().float(), fp.contiguous().float(), mp.contiguous().float()
    fx = None
    if flags.get("use_fx_bus", True):
        from mst.filter import octave_band_filterbank

        noise = fx_noise.contiguous().float()
        assert tuple(noise.shape) == (bs * 2, 12, fx_ir_samples + fx_bandpass_taps - 1)
        filters = octave_band_filterbank(fx_bandpass_taps, sample_rate).contiguous()
        tables = torch.zeros(L.mst_console_fx_tables_bytes() // 4)
        L.mst_console_fx_init_tables(tables, None)
        fx = _cabi.ConsoleFx(noise.data_ptr(), filters.data_ptr(), tables.data_ptr())
    L.mst_console_forward(d, tracks, tp, fp, mp, fx, mix, mixed, status, ws, nbytes, None)
    out = dict(mix=mix, mixed=mixed, status=int(status.item()))
    if grad_mix is not None:
        gtp = torch.full((bs, T, 27), float("nan"))
        gmp = torch.full((bs, 26), float("nan"))
        gtr = torch.zeros(bs, T, n) if want_grad_tracks else None
        gm = grad_mix.contiguous().float()
        gmx = None if grad_mixed is None else grad_mixed.contiguous().float()
        gfp = torch.full((bs, 25), float("nan")) if fx is not None else None
        L.mst_console_backward(d, tracks, tp, fp, mp, fx, gm, gmx, gtp, gfp, gmp, gtr, status, ws, nbytes, None)
        out.update(grad_tp=gtp, grad_mp=gmp, grad_tracks=gtr, grad_fp=gfp, status=int(status.item()))
    return out


def mrstft(pred, target, resolutions, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, sc_per_example=True, grad=True):
    """(bs, chs, n) CPU tensors -> dict(loss, grad_pred)."""
    from mst.loss import _mrstft_desc

    L = lib()
    x = pred.reshape(-1, pred.shape[-1]).contiguous().float()
    y = target.reshape(-1, target.shape[-1]).contiguous().float()
    d = _mrstft_desc(x.shape[0], x.shape[1], resolutions, w_sc, w_log_mag, w_lin_mag, sc_per_example, 1e-8)
    tb, wb = L.mst_mrstft_tables_bytes(d), L.mst_mrstft_workspace_bytes(d)
    assert tb > 0 and wb > 0
    tables = _nan(tb // 4)
    ws = _workspace(wb, float("nan"))  # the product allocates with torch.empty: the kernels must not rely on a cleared workspace
    L.mst_mrstft_init_tables(d, tables, None)
    loss = torch.zeros(1)
    L.mst_mrstft_forward(d, x, y, tables, loss, ws, wb, None)
    out = dict(loss=loss.clone())
    if grad:
        gl = torch.ones(1)
        gx = torch.full_like(x, float("nan"))
        L.mst_mrstft_backward(d, x, y, tables, gl, gx, ws, wb, None)
        out["grad_pred"] = gx.view_as(pred)
    return out


def afloss(pred, target, weights, sample_rate=44100, grad=True, grad_losses=None):
    """(bs, 2, n) CPU tensors -> dict(losses (5,), grad_pred)."""
    from mst.filter import barkscale_fbanks

    L = lib()
    x, y = pred.contiguous().float(), target.contiguous().float()
    bs, _, n = x.shape
    tables = torch.zeros(L.mst_afloss_tables_bytes() // 4)
    L.mst_afloss_init_tables(tables, None)
    fb = barkscale_fbanks(16385, 20.0, 20000.0, 24, sample_rate).contiguous()
    wb = L.mst_afloss_workspace_bytes(bs, n)
    assert wb > 0
    ws = torch.zeros(wb // 4)
    w = (C.c_float * 5)(*weights)
    losses = torch.zeros(5)
    L.mst_afloss_forward(x, y, bs, n, w, tables, fb, losses, ws, wb, None)
    out = dict(losses=losses.clone())
    if grad:
        g = torch.ones(5) if grad_losses is None else grad_losses.float()
        gx = torch.full_like(x, float("nan"))
        L.mst_afloss_backward(x, y, bs, n, w, tables, fb, g, gx, ws, wb, None)
        out["grad_pred"] = gx
    return out


def _ctrl_setup(encoder, bs, seq):
    """-> (desc, [(name, fp32 tensor)] layer-major in mst_ctrl_layer order, NaN workspace, its size in bytes)"""
    from diffmst_hip import controller

    d = controller._desc(encoder, bs, seq)
    sd = encoder.state_dict()
    params = [(f"layers.{l}.{n}", sd[f"layers.{l}.{n}"].detach().float().contiguous()) for l in range(len(encoder.layers))
              for n in controller._PARAM_NAMES]
    nbytes = lib().mst_ctrl_workspace_bytes(d)
    assert nbytes > 0, "encoder stack outside the kernels' limits"
    return d, params, _workspace(nbytes, float("nan")), nbytes  # the kernels must not rely on a cleared workspace


def ctrl_stack(encoder, tokens, mask=None, grad_out=None):
    """``mst_ctrl_forward`` / ``mst_ctrl_backward`` on a CPU ``nn.TransformerEncoder``'s weights.  tokens (bs, S, d), mask (bs, S) with
    non-zero = padded key or None, grad_out (bs, S, d) or None (forward only) -> dict(out, grad_tokens, grads {parameter name: tensor}).
    Every output and gradient buffer starts as NaN: an element no kernel writes fails any comparison."""
    from diffmst_hip.controller import _layer_array, _mask_bytes

    L = lib()
    bs, S, _ = tokens.shape
    d, params, ws, nbytes = _ctrl_setup(encoder, bs, S)
    ps = [p for _, p in params]
    x = tokens.detach().float().contiguous()
    m = _mask_bytes(mask)
    out = _nan(*x.shape)
    L.mst_ctrl_forward(d, x, m, _layer_array(ps, d.n_layers), out, ws, nbytes, None)
    res = dict(out=out)
    if grad_out is not None:
        g = grad_out.detach().float().contiguous()
        grads = [_nan(*p.shape) for p in ps]
        gx = _nan(*x.shape)
        L.mst_ctrl_backward(d, x, _layer_array(ps, d.n_layers), g, _layer_array(grads, d.n_layers), gx, ws, nbytes, None)
        res.update(grad_tokens=gx, grads={n: t for (n, _), t in zip(params, grads)})
    return res


def controller(ctrl, track_embeds, mix_embeds, mask=None, g_t=None, g_f=None, g_m=None):
    """The whole ``TransformerController.forward`` and its backward through the C ABI (``mst_ctrl_tokens_forward``, ``mst_ctrl_forward``,
    ``mst_ctrl_heads_forward`` and their backwards) on a CPU controller's weights.  g_t None = forward only; g_f / g_m None = no gradient
    on that head (its projection gradients are then left as the kernels found them: NaN).
    -> dict(out_t, out_f, out_m, mask_ext, grad_track_embeds, grad_mix_embeds, grads {parameter name: tensor})."""
    from diffmst_hip.controller import _IO_NAMES, _io_struct, _layer_array, _mask_bytes

    L = lib()
    bs, T, D = track_embeds.shape
    enc = ctrl.transformer_encoder
    d, params, ws, nbytes = _ctrl_setup(enc, bs, T + 4)
    ps = [p for _, p in params]
    sd = ctrl.state_dict()
    io = [sd[n].detach().float().contiguous() for n in _IO_NAMES]
    nt, nf, nm = io[4].shape[0], io[6].shape[0], io[8].shape[0]

    te, me = track_embeds.detach().float().contiguous(), mix_embeds.detach().float().contiguous()
    m_in = _mask_bytes(mask)
    tokens, z = _nan(bs, T + 4, D), _nan(bs, T + 4, D)
    m_ext = torch.full((bs, T + 4), 0xAA, dtype=torch.uint8) if mask is not None else None
    out_t, out_f, out_m = _nan(bs, T, nt), _nan(bs, nf), _nan(bs, nm)
    io_s = _io_struct(io)
    L.mst_ctrl_tokens_forward(d, T, te, me, m_in, io_s, tokens, m_ext, None)
    L.mst_ctrl_forward(d, tokens, m_ext, _layer_array(ps, d.n_layers), z, ws, nbytes, None)
    L.mst_ctrl_heads_forward(d, T, z, io_s, nt, nf, nm, out_t, out_f, out_m, None)
    res = dict(out_t=out_t, out_f=out_f, out_m=out_m, mask_ext=m_ext, tokens=tokens, z=z)
    if g_t is None:
        return res
    f32 = lambda g: None if g is None else g.detach().float().contiguous()
    g_t, g_f, g_m = f32(g_t), f32(g_f), f32(g_m)
    io_g = [_nan(*p.shape) for p in io]
    layer_g = [_nan(*p.shape) for p in ps]
    gz, gtok = _nan(*z.shape), _nan(*tokens.shape)
    sbytes = L.mst_ctrl_heads_scratch_bytes(d, T)
    assert sbytes > 0
    scratch = _nan(sbytes // 4)
    iog_s = _io_struct(io_g)
    L.mst_ctrl_heads_backward(d, T, z, io_s, nt, nf, nm, out_t, out_f, out_m, g_t, g_f, g_m, iog_s, gz, scratch, None)
    L.mst_ctrl_backward(d, tokens, _layer_array(ps, d.n_layers), gz, _layer_array(layer_g, d.n_layers), gtok, ws, nbytes, None)
    L.mst_ctrl_tokens_backward(d, T, gtok, iog_s, None)
    grads = {n: g.view_as(sd[n]) for n, g in zip(_IO_NAMES, io_g)}
    grads.update({"transformer_encoder." + n: t for (n, _), t in zip(params, layer_g)})
    res.update(grad_track_embeds=gtok[:, :T], grad_mix_embeds=gtok[:, T:T + 2], grad_z=gz, grads=grads)
    return res
