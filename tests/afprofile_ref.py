"""The shared cases of the feature-profile tests (tests/test_afprofile_hostsim.py on the host simulator, tests/test_afprofile_gpu.py on
the device).

TEST INFRASTRUCTURE.  Defined here once so that the two files cannot drift apart:

* ``Driver``: ``mst_af_profile`` / ``mst_afloss_forward_profile`` / ``mst_afloss_backward_profile`` through the C ABI of a bound
  library, on the host (simulator library) or on the device (product library).  Every output starts as NaN between guard regions, the
  workspace as NaN too: an element no kernel writes fails any comparison, a kernel that relies on a cleared workspace returns NaN.
* ``references``: the float64 and the fp32 evaluation of ``oracle.loss_restated.audio_feature_loss`` - which takes an input and a
  target of different lengths, as the reference's class does - computed once per case, shared and never modified.
* ``check_*``: the cases.  The bounds are the project's own three-way forms (tests/test_loss_gpu.py): the kernels may sit no further
  from float64 than three times what the fp32 evaluation of the same formulas does, plus 2e-5.
"""
import ctypes
import functools
import os

import numpy as np
import torch

from oracle import loss_restated as ol
from util import rel

GUARD = 64
AF_WEIGHTS = [0.1, 0.001, 1.0, 1.0, 0.1]  # reference configs/models/unpaired+feat.yaml:55-60
COTANGENT = [1.0, 2.0, 0.5, 1.5, 1.0]     # of tests/test_loss_gpu.py::test_afloss_three_way
NP = 54
FEATS = (("rms", ol.feat_rms), ("crest_factor", ol.feat_crest_factor), ("stereo_width", ol.feat_stereo_width),
         ("stereo_imbalance", ol.feat_stereo_imbalance), ("barkspectrum", ol.feat_barkspectrum))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Driver:
    """``lib``: a bound library; ``device``: where its kernels read and write ("cpu" for the simulator)."""

    def __init__(self, lib, device, sample_rate=44100):
        from mst.filter import barkscale_fbanks

        self.lib, self.device = lib, torch.device(device)
        self._all = []
        self.tables = torch.zeros(lib.mst_afloss_tables_bytes() // 4, device=self.device)
        lib.mst_afloss_init_tables(self.tables, self.stream_ptr())
        self.fb = barkscale_fbanks(16385, 20.0, 20000.0, 24, sample_rate).contiguous().to(self.device)

    def stream_ptr(self):
        if self.device.type == "cpu":
            return None
        from mst import _hip

        return _hip.current_stream_ptr(self.device)

    def guarded(self, n, dtype=torch.float32):
        """n NaNs with GUARD more on either side -> the inner view; ``check_guards`` looks at every buffer handed out."""
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=self.device)
        self._all.append((buf, n))
        return buf[GUARD:GUARD + n]

    def check_guards(self):
        for buf, n in self._all:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "written outside a buffer"

    def workspace(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        ws = torch.full((nbytes // 4 + 64,), float("nan"), device=self.device)
        return ws[(-ws.data_ptr() % 256) // 4:]  # on a 256-byte boundary like a device allocation

    def profile(self, x):
        """x (bs, 2, n) host tensor -> (bs, 54) float64 on the driver's device."""
        x = x.float().contiguous().to(self.device)
        bs, _, n = x.shape
        nbytes = self.lib.mst_af_profile_workspace_bytes(bs, n)
        out = self.guarded(bs * NP, torch.float64)
        self.lib.mst_af_profile(x, bs, n, self.tables, self.fb, out, self.workspace(nbytes), nbytes, self.stream_ptr())
        return out.view(bs, NP)

    def loss(self, pred, profile, weights, grad_losses=None):
        """pred (bs, 2, n) host tensor, profile (bs, 54) on the device -> dict(losses (5,), grad_pred (bs, 2, n)) on the host."""
        x = pred.float().contiguous().to(self.device)
        bs, _, n = x.shape
        nbytes = self.lib.mst_afloss_profile_workspace_bytes(bs, n)
        ws = self.workspace(nbytes)
        w = (ctypes.c_float * 5)(*weights)
        losses = self.guarded(5)
        prof = profile.contiguous()
        self.lib.mst_afloss_forward_profile(x, prof, bs, n, w, self.tables, self.fb, losses, ws, nbytes, self.stream_ptr())
        out = dict(losses=losses.cpu().clone())
        if grad_losses is not None:
            g = torch.tensor(grad_losses, dtype=torch.float32).to(self.device)
            gx = self.guarded(x.numel())
            self.lib.mst_afloss_backward_profile(x, prof, bs, n, w, self.tables, self.fb, g, gx, ws, nbytes, self.stream_ptr())
            out["grad_pred"] = gx.view_as(x).cpu().clone()
        return out


def profile_object(data, sample_rate=44100):
    """The package's view of a driver's profile (its feature views are torch operations on the 54 numbers: any device)."""
    from mst.loss import AudioFeatureProfile

    return AudioFeatureProfile(data.clone(), sample_rate)


def views(profile):
    return {name: getattr(profile, name).double().cpu() for name, _ in FEATS}


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- case 1: unequal lengths, three-way -------------------------------------------------------------------------------------------
def signals(bs, n_pred, n_target):
    """The draws of test_afloss_three_way, the target with its own length."""
    torch.manual_seed(n_pred + bs)
    x = 0.2 * torch.randn(bs, 2, n_pred)
    x[:, 1] = 0.6 * x[:, 1] + 0.3 * x[:, 0]
    y = 0.3 * torch.randn(bs, 2, n_target) * torch.tensor([1.0, 0.5]).view(1, 2, 1)
    return x, y


@functools.lru_cache(maxsize=None)
def references(bs, n_pred, n_target):
    """(x, y, {dtype: (five losses as float64, gradient)}) of a case: computed once, shared, never modified."""
    x, y = signals(bs, n_pred, n_target)
    gw = torch.tensor(COTANGENT)
    res = {}
    for dt in (torch.float32, torch.float64):
        xo = x.clone().to(dt).requires_grad_(True)
        lo = ol.audio_feature_loss(xo, y.to(dt), AF_WEIGHTS)
        vo = torch.stack([lo[k] for k in ol.AF_KEYS])
        (vo * gw.to(dt)).sum().backward()
        res[dt] = (vo.detach().double(), xo.grad)
    return x, y, res


def assert_three_way(tag, losses, grad, res, record=None):
    v64, g64 = res[torch.float64]
    v32, g32 = res[torch.float32]
    err = (losses.double() - v64).abs() / v64.abs().clamp_min(1e-30)
    err32 = (v32 - v64).abs() / v64.abs().clamp_min(1e-30)
    e_g, e_g32 = rel(grad, g64), rel(g32, g64)
    print(f"\n[af profile {tag}] loss rel err hip {err.tolist()} ref32 {err32.tolist()}; grad hip-f64 {e_g:.2e} ref32-f64 {e_g32:.2e}")
    if record is not None:
        record(loss_rel_err_hip_vs_f64=err.tolist(), loss_rel_err_ref32_vs_f64=err32.tolist(), grad=(rel(grad, g32), e_g, e_g32))
    assert bool(torch.isfinite(grad).all())
    assert (err <= 3 * err32 + 2e-5).all()
    assert e_g <= 3 * e_g32 + 2e-5


def check_three_way(drv, bs, n_pred, n_target, record=None):
    x, y, res = references(bs, n_pred, n_target)
    out = drv.loss(x, drv.profile(y), AF_WEIGHTS, COTANGENT)
    drv.check_guards()
    assert_three_way(f"{bs}x2x{n_pred} vs {n_target}", out["losses"], out["grad_pred"], res, record)


# ---- cases 2 and 3: the fixtures the reference's own class and functions wrote ---------------------------------------------------------
def assert_golden(g, losses, grad, truth, record=None):
    """The assertions of tests/test_loss_gpu.py::test_afloss_golden: ``losses`` (5,) and ``grad`` of sum(v.mean())."""
    for i, k in enumerate(ol.AF_KEYS):
        got, ref, t64 = losses[i].item(), float(g["loss." + k]), truth[k].item()
        assert abs(got - ref) <= 5e-5 * abs(ref) + 1e-12, (k, got, ref)
        assert abs(got - t64) <= 2 * abs(ref - t64) + 1e-5 * abs(t64), (k, got, ref, t64)
    gsub = torch.from_numpy(g["grad_input_sub"])
    e = rel(grad[..., ::16], gsub)
    if record is not None:
        record(grad_vs_reference=e, **{k.replace("-", "_"): abs(losses[i].item() - float(g["loss." + k])) / abs(float(g["loss." + k]))
                                       for i, k in enumerate(ol.AF_KEYS)})
    assert e < 2e-4
    assert abs(grad.double().pow(2).sum().sqrt().item() - float(g["grad_input_l2"])) / float(g["grad_input_l2"]) < 2e-4


def assert_features(tag, got, fixture, x, record=None):
    """Per feature tensor: rel(hip, f64) <= 3 rel(fixture, f64) + 2e-5, float64 oracle features of ``x`` as truth."""
    for name, fn in FEATS:
        t64 = fn(x.double())
        assert got[name].shape == t64.shape == fixture[name].shape, (name, got[name].shape, t64.shape)
        e, e_fix = rel(got[name], t64), rel(fixture[name].double(), t64)
        print(f"[af profile {tag}] {name}: hip-f64 {e:.2e}  fixture-f64 {e_fix:.2e}")
        if record is not None:
            record(**{name: (e, e_fix)})
        assert e <= 3 * e_fix + 2e-5, (name, e, e_fix)


def check_golden_features(drv, record=None):
    """profile(input)'s five views against what the reference's compute_* functions returned for that input (af_loss.npz)."""
    g = np.load(os.path.join(GOLDEN, "af_loss.npz"))
    x = torch.from_numpy(g["input"])
    got = views(profile_object(drv.profile(x)))
    drv.check_guards()
    fixture = {name: torch.from_numpy(g["feat." + key]) for (name, _), key in zip(FEATS, ("rms", "crest", "width", "imbalance", "bark"))}
    assert_features("golden", got, fixture, x, record)


def check_golden_loss(drv, name, record=None):
    """loss(input, profile(target)) against the losses and the gradient the reference's class produced."""
    g = np.load(os.path.join(GOLDEN, name))
    x, y, weights = torch.from_numpy(g["input"]), torch.from_numpy(g["target"]), [float(v) for v in g["weights"]]
    out = drv.loss(x, drv.profile(y), weights, [1.0] * 5)  # sum(v.mean() for v in losses.values()), mst/system.py:334-336
    drv.check_guards()
    truth = ol.audio_feature_loss(x.double(), y.double(), weights)
    assert_golden(g, out["losses"], out["grad_pred"], truth, record)


# ---- case 4: known answers -----------------------------------------------------------------------------------------------------------
def check_known_answers(drv, bs=2, n=40000):
    torch.manual_seed(0)
    a = torch.randn(bs, 2, n)
    z = drv.loss(a, drv.profile(a), [1.0] * 5)["losses"]  # both analyses of one signal take one arithmetic route
    assert bool((z.abs() < 1e-10).all()), z.tolist()
    sq = torch.ones(1, 2, n)
    sq[..., ::2] = -1.0  # +-1 square wave: every sum of squares is exact
    p = profile_object(drv.profile(sq))
    assert bool((p.rms.cpu() - 1.0).abs().max() < 1e-6) and bool(p.crest_factor.cpu().abs().max() < 1e-5)
    mono = a.clone()
    mono[:, 1] = mono[:, 0]
    assert bool((profile_object(drv.profile(mono)).stereo_width.cpu() == 0).all())
    left_silent = a.clone()
    left_silent[:, 0] = 0.0
    assert bool((profile_object(drv.profile(left_silent)).stereo_imbalance.cpu() - 1.0).abs().max() < 1e-6)
    drv.check_guards()


# ---- case 5: a long signal (device only: 129 frames) ---------------------------------------------------------------------------------
def check_long(drv, n=1048579, record=None):
    torch.manual_seed(5)
    x = 0.2 * torch.randn(1, 2, n)
    x[:, 1] = 0.6 * x[:, 1] + 0.3 * x[:, 0]
    got = views(profile_object(drv.profile(x)))
    drv.check_guards()
    fp32 = {name: fn(x) for name, fn in FEATS}  # what a second fp32 evaluation of the formulas gives
    assert_features(f"1x2x{n}", got, fp32, x, record)


# ---- case 6: determinism and bounds of writes ----------------------------------------------------------------------------------------
def check_determinism_and_bounds(drv, bs, n_pred, n_target):
    x, y = signals(bs, n_pred, n_target)
    runs = []
    for _ in range(2):
        prof = drv.profile(y)
        assert bool(torch.isfinite(prof).all()), "profile not fully written"
        out = drv.loss(x, prof, AF_WEIGHTS, COTANGENT)
        assert bool(torch.isfinite(out["losses"]).all()) and bool(torch.isfinite(out["grad_pred"]).all()), "an output element was not written"
        runs.append((prof.cpu().clone(), out["losses"], out["grad_pred"]))
    drv.check_guards()  # exactly bs * 54 doubles, 5 losses and bs * 2 * n gradient elements between untouched guards
    for a, b in zip(*runs):
        assert torch.equal(bits(a), bits(b))


# ---- case 7: validation --------------------------------------------------------------------------------------------------------------
def check_validation(drv):
    from mst import _cabi

    L, st = drv.lib, drv.stream_ptr()
    for name in ("mst_af_profile_workspace_bytes", "mst_af_profile", "mst_afloss_profile_workspace_bytes", "mst_afloss_forward_profile",
                 "mst_afloss_backward_profile"):
        assert hasattr(L, name) and name in _cabi.SIGNATURES
    assert L.mst_abi_version() == _cabi.ABI_VERSION == 13 and _cabi.AF_PROFILE_DOUBLES == NP
    for size in (L.mst_af_profile_workspace_bytes, L.mst_afloss_profile_workspace_bytes):
        assert size(1, 16384) == 0 and size(0, 20000) == 0 and size(-1, 20000) == 0 and size(1, 16385) > 0
    # the one-set plan counts its own units: never more workspace than the paired loss takes
    assert L.mst_af_profile_workspace_bytes(2, 40000) < L.mst_afloss_profile_workspace_bytes(2, 40000) < L.mst_afloss_workspace_bytes(2, 40000)
    bs, n = 1, 17000
    x = torch.zeros(bs, 2, n, device=drv.device)
    prof, losses, gx = drv.guarded(bs * NP, torch.float64), drv.guarded(5), drv.guarded(bs * 2 * n)
    g = torch.ones(5, device=drv.device)
    w = (ctypes.c_float * 5)(*AF_WEIGHTS)
    nb_p, nb_l = L.mst_af_profile_workspace_bytes(bs, n), L.mst_afloss_profile_workspace_bytes(bs, n)
    ws = drv.workspace(nb_l)

    def refused(fn, *args):
        try:
            fn(*args)
        except _cabi.AbiError as e:
            assert e.code != 0
            return
        raise AssertionError(f"{fn.__name__} accepted {args}")

    good = dict(x=x, bs=bs, n=n, tables=drv.tables, fb=drv.fb, prof=prof, ws=ws, w=w, losses=losses, g=g, gx=gx)
    for change in (dict(n=16384), dict(bs=0), dict(x=None), dict(tables=None), dict(fb=None), dict(prof=None), dict(ws=None)):
        a = dict(good, **change)
        refused(L.mst_af_profile, a["x"], a["bs"], a["n"], a["tables"], a["fb"], a["prof"], a["ws"], nb_p, st)
    refused(L.mst_af_profile, x, bs, n, drv.tables, drv.fb, prof, ws, nb_p - 4, st)
    for change in (dict(n=16384), dict(bs=0), dict(x=None), dict(prof=None), dict(w=None), dict(tables=None), dict(fb=None),
                   dict(losses=None), dict(ws=None)):
        a = dict(good, **change)
        refused(L.mst_afloss_forward_profile, a["x"], a["prof"], a["bs"], a["n"], a["w"], a["tables"], a["fb"], a["losses"], a["ws"], nb_l, st)
    for change in (dict(n=16384), dict(bs=0), dict(x=None), dict(prof=None), dict(w=None), dict(tables=None), dict(fb=None), dict(g=None),
                   dict(gx=None), dict(ws=None)):
        a = dict(good, **change)
        refused(L.mst_afloss_backward_profile, a["x"], a["prof"], a["bs"], a["n"], a["w"], a["tables"], a["fb"], a["g"], a["gx"], a["ws"],
                nb_l, st)
    for t in (prof, losses, gx, ws):
        assert bool(torch.isnan(t).all()), "a refused call wrote something"
    drv.check_guards()
