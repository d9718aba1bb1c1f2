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
    nbytes = L.mst_console_workspace_bytes(C.byref(d))
    assert nbytes > 0
    ws = torch.zeros(nbytes // 4 + 64, dtype=torch.float32)
    off = (-ws.data_ptr() % 256) // 4
    ws = ws[off:]
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
        assert L.mst_console_fx_init_tables(_cabi.ptr(tables), None) == 0
        fx = _cabi.ConsoleFx(noise.data_ptr(), filters.data_ptr(), tables.data_ptr())
    fxp = C.byref(fx) if fx is not None else None
    rc = L.mst_console_forward(C.byref(d), _cabi.ptr(tracks), _cabi.ptr(tp), _cabi.ptr(fp), _cabi.ptr(mp), fxp, _cabi.ptr(mix),
                               _cabi.ptr(mixed), _cabi.ptr(status), _cabi.ptr(ws), nbytes, None)
    assert rc == 0, rc
    out = dict(mix=mix, mixed=mixed, status=int(status.item()))
    if grad_mix is not None:
        gtp = torch.full((bs, T, 27), float("nan"))
        gmp = torch.full((bs, 26), float("nan"))
        gtr = torch.zeros(bs, T, n) if want_grad_tracks else None
        gm = grad_mix.contiguous().float()
        gmx = None if grad_mixed is None else grad_mixed.contiguous().float()
        gfp = torch.full((bs, 25), float("nan")) if fx is not None else None
        rc = L.mst_console_backward(C.byref(d), _cabi.ptr(tracks), _cabi.ptr(tp), _cabi.ptr(fp), _cabi.ptr(mp), fxp, _cabi.ptr(gm),
                                    _cabi.ptr(gmx), _cabi.ptr(gtp), _cabi.ptr(gfp), _cabi.ptr(gmp), _cabi.ptr(gtr), _cabi.ptr(status),
                                    _cabi.ptr(ws), nbytes, None)
        assert rc == 0, rc
        out.update(grad_tp=gtp, grad_mp=gmp, grad_tracks=gtr, grad_fp=gfp, status=int(status.item()))
    return out


def mrstft(pred, target, resolutions, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, sc_per_example=True, grad=True):
    """(bs, chs, n) CPU tensors -> dict(loss, grad_pred)."""
    from mst import _cabi

    L = lib()
    x = pred.reshape(-1, pred.shape[-1]).contiguous().float()
    y = target.reshape(-1, target.shape[-1]).contiguous().float()
    d = _cabi.MrstftDesc()
    d.rows, d.n_samples, d.n_res = x.shape[0], x.shape[1], len(resolutions)
    for i, (nf, hop, win) in enumerate(resolutions):
        d.fft_size[i], d.hop_size[i], d.win_length[i] = nf, hop, win
    d.w_sc, d.w_log_mag, d.w_lin_mag = w_sc, w_log_mag, w_lin_mag
    d.sc_per_example, d.eps = int(sc_per_example), 1e-8
    tb, wb = L.mst_mrstft_tables_bytes(C.byref(d)), L.mst_mrstft_workspace_bytes(C.byref(d))
    assert tb > 0 and wb > 0
    tables = torch.zeros(tb // 4)
    ws = torch.zeros(wb // 4)
    assert L.mst_mrstft_init_tables(C.byref(d), _cabi.ptr(tables), None) == 0
    loss = torch.zeros(1)
    assert L.mst_mrstft_forward(C.byref(d), _cabi.ptr(x), _cabi.ptr(y), _cabi.ptr(tables), _cabi.ptr(loss), _cabi.ptr(ws), wb, None) == 0
    out = dict(loss=loss.clone())
    if grad:
        gl = torch.ones(1)
        gx = torch.full_like(x, float("nan"))
        assert L.mst_mrstft_backward(C.byref(d), _cabi.ptr(x), _cabi.ptr(y), _cabi.ptr(tables), _cabi.ptr(gl), _cabi.ptr(gx),
                                     _cabi.ptr(ws), wb, None) == 0
        out["grad_pred"] = gx.view_as(pred)
    return out


def afloss(pred, target, weights, sample_rate=44100, grad=True, grad_losses=None):
    """(bs, 2, n) CPU tensors -> dict(losses (5,), grad_pred)."""
    from mst import _cabi
    from mst.filter import barkscale_fbanks

    L = lib()
    x, y = pred.contiguous().float(), target.contiguous().float()
    bs, _, n = x.shape
    tables = torch.zeros(L.mst_afloss_tables_bytes() // 4)
    assert L.mst_afloss_init_tables(_cabi.ptr(tables), None) == 0
    fb = barkscale_fbanks(16385, 20.0, 20000.0, 24, sample_rate).contiguous()
    wb = L.mst_afloss_workspace_bytes(bs, n)
    assert wb > 0
    ws = torch.zeros(wb // 4)
    w = (C.c_float * 5)(*weights)
    losses = torch.zeros(5)
    assert L.mst_afloss_forward(_cabi.ptr(x), _cabi.ptr(y), bs, n, w, _cabi.ptr(tables), _cabi.ptr(fb), _cabi.ptr(losses),
                                _cabi.ptr(ws), wb, None) == 0
    out = dict(losses=losses.clone())
    if grad:
        g = torch.ones(5) if grad_losses is None else grad_losses.float()
        gx = torch.full_like(x, float("nan"))
        assert L.mst_afloss_backward(_cabi.ptr(x), _cabi.ptr(y), bs, n, w, _cabi.ptr(tables), _cabi.ptr(fb), _cabi.ptr(g),
                                     _cabi.ptr(gx), _cabi.ptr(ws), wb, None) == 0
        out["grad_pred"] = gx
    return out


_CTRL_LAYER_NAMES = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                     "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                     "norm2.bias")  # mst_ctrl_layer order
_CTRL_IO_NAMES = ("track_embedding", "mix_embedding", "fx_bus_embedding", "master_bus_embedding", "track_projection.weight",
                  "track_projection.bias", "fx_bus_projection.weight", "fx_bus_projection.bias", "master_bus_projection.weight",
                  "master_bus_projection.bias")  # mst_ctrl_io order


def _nan(*shape):
    return torch.full(shape, float("nan"))


def _ctrl_setup(encoder, bs, seq):
    """-> (desc, [(name, fp32 tensor)] layer-major in mst_ctrl_layer order, NaN workspace, its size in bytes)"""
    from mst import _cabi

    layer = encoder.layers[0]
    d = _cabi.CtrlDesc(bs, seq, layer.self_attn.embed_dim, layer.self_attn.num_heads, layer.linear1.out_features, len(encoder.layers),
                       float(layer.norm1.eps))
    sd = encoder.state_dict()
    params = [(f"layers.{l}.{n}", sd[f"layers.{l}.{n}"].detach().float().contiguous()) for l in range(len(encoder.layers))
              for n in _CTRL_LAYER_NAMES]
    nbytes = lib().mst_ctrl_workspace_bytes(C.byref(d))
    assert nbytes > 0, "encoder stack outside the kernels' limits"
    ws = _nan(nbytes // 4 + 64)  # the kernels must not rely on a cleared workspace
    ws = ws[(-ws.data_ptr() % 256) // 4:]
    return d, params, ws, nbytes


def _ctrl_layer_array(tensors, n_layers):
    from mst import _cabi

    arr = (_cabi.CtrlLayer * n_layers)()
    k = len(_cabi.CTRL_FIELDS)
    for l in range(n_layers):
        for j, name in enumerate(_cabi.CTRL_FIELDS):
            setattr(arr[l], name, tensors[l * k + j].data_ptr())
    return arr


def _ctrl_mask(mask):
    return None if mask is None else (mask != 0).to(torch.uint8).contiguous()


def ctrl_stack(encoder, tokens, mask=None, grad_out=None):
    """``mst_ctrl_forward`` / ``mst_ctrl_backward`` on a CPU ``nn.TransformerEncoder``'s weights.  tokens (bs, S, d), mask (bs, S) with
    non-zero = padded key or None, grad_out (bs, S, d) or None (forward only) -> dict(out, grad_tokens, grads {parameter name: tensor}).
    Every output and gradient buffer starts as NaN: an element no kernel writes fails any comparison."""
    from mst import _cabi

    L = lib()
    bs, S, _ = tokens.shape
    d, params, ws, nbytes = _ctrl_setup(encoder, bs, S)
    ps = [p for _, p in params]
    x = tokens.detach().float().contiguous()
    m = _ctrl_mask(mask)
    out = _nan(*x.shape)
    rc = L.mst_ctrl_forward(C.byref(d), _cabi.ptr(x), _cabi.ptr(m), _ctrl_layer_array(ps, d.n_layers), _cabi.ptr(out), _cabi.ptr(ws), nbytes,
                            None)
    assert rc == 0, rc
    res = dict(out=out)
    if grad_out is not None:
        g = grad_out.detach().float().contiguous()
        grads = [_nan(*p.shape) for p in ps]
        gx = _nan(*x.shape)
        rc = L.mst_ctrl_backward(C.byref(d), _cabi.ptr(x), _ctrl_layer_array(ps, d.n_layers), _cabi.ptr(g),
                                 _ctrl_layer_array(grads, d.n_layers), _cabi.ptr(gx), _cabi.ptr(ws), nbytes, None)
        assert rc == 0, rc
        res.update(grad_tokens=gx, grads={n: t for (n, _), t in zip(params, grads)})
    return res


def controller(ctrl, track_embeds, mix_embeds, mask=None, g_t=None, g_f=None, g_m=None):
    """The whole ``TransformerController.forward`` and its backward through the C ABI (``mst_ctrl_tokens_forward``, ``mst_ctrl_forward``,
    ``mst_ctrl_heads_forward`` and their backwards) on a CPU controller's weights.  g_t None = forward only; g_f / g_m None = no gradient
    on that head (its projection gradients are then left as the kernels found them: NaN).
    -> dict(out_t, out_f, out_m, mask_ext, grad_track_embeds, grad_mix_embeds, grads {parameter name: tensor})."""
    from mst import _cabi

    L = lib()
    bs, T, D = track_embeds.shape
    enc = ctrl.transformer_encoder
    d, params, ws, nbytes = _ctrl_setup(enc, bs, T + 4)
    ps = [p for _, p in params]
    sd = ctrl.state_dict()
    io = [sd[n].detach().float().contiguous() for n in _CTRL_IO_NAMES]
    nt, nf, nm = io[4].shape[0], io[6].shape[0], io[8].shape[0]

    def io_struct(tensors):
        s = _cabi.CtrlIO()
        for name, t in zip(_cabi.CTRL_IO_FIELDS, tensors):
            setattr(s, name, t.data_ptr() if t is not None else None)
        return s

    te, me = track_embeds.detach().float().contiguous(), mix_embeds.detach().float().contiguous()
    m_in = _ctrl_mask(mask)
    tokens, z = _nan(bs, T + 4, D), _nan(bs, T + 4, D)
    m_ext = torch.full((bs, T + 4), 0xAA, dtype=torch.uint8) if mask is not None else None
    out_t, out_f, out_m = _nan(bs, T, nt), _nan(bs, nf), _nan(bs, nm)
    io_s = io_struct(io)
    rc = L.mst_ctrl_tokens_forward(C.byref(d), T, _cabi.ptr(te), _cabi.ptr(me), _cabi.ptr(m_in), C.byref(io_s), _cabi.ptr(tokens),
                                   _cabi.ptr(m_ext), None)
    assert rc == 0, rc
    rc = L.mst_ctrl_forward(C.byref(d), _cabi.ptr(tokens), _cabi.ptr(m_ext), _ctrl_layer_array(ps, d.n_layers), _cabi.ptr(z), _cabi.ptr(ws),
                            nbytes, None)
    assert rc == 0, rc
    rc = L.mst_ctrl_heads_forward(C.byref(d), T, _cabi.ptr(z), C.byref(io_s), nt, nf, nm, _cabi.ptr(out_t), _cabi.ptr(out_f), _cabi.ptr(out_m),
                                  None)
    assert rc == 0, rc
    res = dict(out_t=out_t, out_f=out_f, out_m=out_m, mask_ext=m_ext, tokens=tokens, z=z)
    if g_t is None:
        return res
    f32 = lambda g: None if g is None else g.detach().float().contiguous()
    g_t, g_f, g_m = f32(g_t), f32(g_f), f32(g_m)
    io_g = [_nan(*p.shape) for p in io]
    layer_g = [_nan(*p.shape) for p in ps]
    gz, gtok = _nan(*z.shape), _nan(*tokens.shape)
    sbytes = L.mst_ctrl_heads_scratch_bytes(C.byref(d), T)
    assert sbytes > 0
    scratch = _nan(sbytes // 4)
    iog_s = io_struct(io_g)
    rc = L.mst_ctrl_heads_backward(C.byref(d), T, _cabi.ptr(z), C.byref(io_s), nt, nf, nm, _cabi.ptr(out_t), _cabi.ptr(out_f), _cabi.ptr(out_m),
                                   _cabi.ptr(g_t), _cabi.ptr(g_f), _cabi.ptr(g_m), C.byref(iog_s), _cabi.ptr(gz), _cabi.ptr(scratch), None)
    assert rc == 0, rc
    rc = L.mst_ctrl_backward(C.byref(d), _cabi.ptr(tokens), _ctrl_layer_array(ps, d.n_layers), _cabi.ptr(gz),
                             _ctrl_layer_array(layer_g, d.n_layers), _cabi.ptr(gtok), _cabi.ptr(ws), nbytes, None)
    assert rc == 0, rc
    rc = L.mst_ctrl_tokens_backward(C.byref(d), T, _cabi.ptr(gtok), C.byref(iog_s), None)
    assert rc == 0, rc
    grads = {n: g.view_as(sd[n]) for n, g in zip(_CTRL_IO_NAMES, io_g)}
    grads.update({"transformer_encoder." + n: t for (n, _), t in zip(params, layer_g)})
    res.update(grad_track_embeds=gtok[:, :T], grad_mix_embeds=gtok[:, T:T + 2], grad_z=gz, grads=grads)
    return res
