"""The MR-STFT loss on every transform size and dispatch route: the case table, the input recipe and the grading shared by
tests/test_mrstft_routes_gpu.py (the device) and tests/test_mrstft_routes_hostsim.py (the host simulator).  A plain module, no conftest.

Which kernels a call runs is decided per resolution by `make_plan` and `mst_mrstft_backward` (diff-mst_amd/csrc/mst_stft.hip):
  * a resolution runs on the register-radix ("fast") kernels of mst_stft2.hip when n_fft is 512 / 2048 / 8192, hop = n_fft / 2, the
    window is full, n % hop == 0 and n >= 2 n_fft - and, of several 8192-point resolutions that qualify, only the first; every other
    resolution runs on the generic LDS kernels of mst_stft.hip (any power of two 128..8192, any hop, any window length);
  * the forward of exactly {512, 2048, 8192}, all fast, is ONE launch (k_stft3_fwd); otherwise one launch per resolution;
  * the backward is all-generic (memset + float atomics) as soon as ONE resolution is generic; with all of them fast it is
      "own"   no 8192-point resolution: the first launch owns the gradient buffer, the others add to it
      "zero"  an 8192-point resolution and nothing behind it: memset, then the seam halves are added atomically
      "seam"  one 8192-point resolution and a 512 / 2048 one behind it: the seams travel through a scratch slab, no memset
      "+fused" one 512 and one 2048 resolution, n % 1024 == 0 and n >= 8192: both in one launch (k_stft2_bwd_512_2048).
Each case states the route it means to hit (`fast`, `bwd`); `route_by_rule` restates the rules above so that the table can be checked
against them, and `workspace_floats` restates the plan's workspace layout, through which the C ABI shows which resolutions got the
fast kernels (they keep two planes each) and whether the seam slab exists.

Grading (smooth terms only unless a case says otherwise: the log-magnitude term's 1 / |X| statistics belong to tests/test_loss_gpu.py):
x = 0.3 randn, y = 0.5 x + 0.2 randn, a seed per case; references oracle.loss_restated.mrstft_loss in float64 and in float32.
  loss      |loss - l64| / l64 < 1e-5                                   (the suite's loss bound)
  gradient  h <= 2 r + 1e-5,  h = rel-L2(HIP, f64), r = rel-L2(fp32 oracle, f64)  (test_mrstft_gradient_every_draw_off_the_ill_posed_bins)
  per sample  the same form on max |g - g64| / max |g64|: at these lengths ONE wrong sample moves both figures by 1e-3 or more
  samples no frame reaches (hop >= n_fft) have a gradient of exactly 0, and no element of the result is NaN (the callers start the
  gradient buffer and the workspace as NaN).
"""
import functools
import zlib
from dataclasses import dataclass, field

import torch

R3 = ((512, 256, 512), (2048, 1024, 2048), (8192, 4096, 8192))  # the reference's resolutions (configs/models/naive.yaml)
SMOOTH = dict(w_sc=1.0, w_log_mag=0.0)


@dataclass(frozen=True)
class Case:
    id: str
    res: tuple          # ((n_fft, hop, win_length), ...)
    n: int              # samples per row
    why: str
    rows: tuple = (1, 2)  # (bs, channels)
    fast: str = ""      # per resolution: "F" = register-radix kernels, "g" = generic LDS kernels ("" = all generic)
    bwd: str = "generic"
    kw: dict = field(default_factory=lambda: dict(SMOOTH))
    sim: str = "run"    # host simulator: "run", "slow" (40 s or more there: MST_RUN_SLOW=1 only) or "never" (minutes; device only)

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) & 0xFFFF

    @property
    def n_rows(self):
        return self.rows[0] * self.rows[1]

    @property
    def fast_flags(self):
        return tuple(c == "F" for c in (self.fast or "g" * len(self.res)))


def _one(nf, hop, win):
    return ((nf, hop, win),)


GLOBAL_SC = dict(SMOOTH, sc_per_example=False)
R8, R2K, R5C = R3[2], R3[1], R3[0]

CASES = (
    # ---- generic kernels, every size ---------------------------------------------------------------------------------------------
    Case("g128_n1000", _one(128, 32, 128), 1000, "smallest transform (radix-2 stage + 3 radix-4 stages)"),
    Case("g128_n65", _one(128, 32, 128), 65, "shortest legal row: every frame reflects at both ends"),
    Case("g256_win255_n777", _one(256, 64, 255), 777, "odd window length, odd row length"),
    Case("g1024_hop120_win600_n2001", _one(1024, 120, 600), 2001, "odd centre padding of the window, hop not dividing n_fft"),
    Case("g512_hop128_win333_n3000", _one(512, 128, 333), 3000, "generic 512-point kernels, odd window"),
    Case("g4096_hop1024_n9001", _one(4096, 1024, 4096), 9001, "largest paired backward size, odd frame count (9): last frame unpaired"),
    Case("g4096_hop512_n2049", _one(4096, 512, 4096), 2049, "row one sample longer than the reflect padding"),
    Case("g8192_hop1024_n4097", _one(8192, 1024, 8192), 4097, "generic 8192 (in-place backward), frames that reflect at both ends"),
    Case("g2048_hop256_n1100", _one(2048, 256, 2048), 1100, "frames that reflect at both ends"),
    Case("g512_hop512_n5000", _one(512, 512, 512), 5000, "hop = n_fft: frames tile the row without overlap, its tail past the last frame gets an exact 0 gradient"),
    Case("g512_hop700_n5000", _one(512, 700, 512), 5000, "hop > n_fft: samples between frames get an exact 0 gradient"),
    Case("g256_hop32_rows3x2_n6000", _one(256, 32, 256), 6000, "n_frames * rows >= 1024: two frames per forward workgroup",
         rows=(3, 2), sim="slow"),
    Case("g256_win1_n3000", _one(256, 64, 1), 3000, "win_length 1: torch.hann_window(1) is [1.]"),
    Case("g256_win2_n3000", _one(256, 64, 2), 3000, "win_length 2: the window is [0, 1]"),
    Case("auraloss_default_n30001", ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)), 30001,
         "auraloss' default resolutions, smooth term only: the tight companion of test_mrstft_odd_configuration", sim="slow"),
    Case("g512_g1024_global_sc_rows3x2_n3000", ((512, 128, 400), (1024, 256, 1024)), 3000,
         "batch-global spectral convergence on the generic kernels", rows=(3, 2), kw=GLOBAL_SC),
    Case("g512_g256_lin_mag_n3000", ((512, 256, 512), (256, 50, 200)), 3000, "linear-magnitude L1 term (sign() cotangent) beside SC",
         kw=dict(w_sc=1.0, w_log_mag=0.0, w_lin_mag=1.0)),
    # ---- the reference's resolutions at lengths that are no multiple of 4096: none, one or two of them on the fast kernels ----------
    Case("r3_n4097", R3, 4097, "no resolution qualifies (odd length)", fast="ggg"),
    Case("r3_n4352", R3, 4352, "17 x 256: only 512 qualifies; forward mixed, backward all generic", fast="Fgg"),
    Case("r3_n5120", R3, 5120, "5 x 1024: 512 and 2048 qualify, 8192 is too long for the row", fast="FFg"),
    Case("r3_n16385", R3, 16385, "one sample past the shortest all-fast row: all generic", fast="ggg"),
    Case("r3_n21504", R3, 21504, "21 x 1024, not a multiple of 4096: 8192 generic behind two fast forwards", fast="FFg"),
    Case("r3_8192_first_n21504", (R8, R5C, R2K), 21504, "first launch generic: the loss takes the three-launch finish", fast="gFF"),
    # ---- 512 + 2048, either side of the fused backward's threshold (n % 1024 == 0 and n >= 8192) -------------------------------------
    Case("r2_n4096", R3[:2], 4096, "shortest row the 2048-point fast kernels take", fast="FF", bwd="own"),
    Case("r2_n5120", R3[:2], 5120, "below the fused threshold", fast="FF", bwd="own"),
    Case("r2_n7168", R3[:2], 7168, "last multiple of 1024 below the fused threshold", fast="FF", bwd="own"),
    Case("r2_n8192", R3[:2], 8192, "first length of the fused 512 + 2048 backward", fast="FF", bwd="own+fused"),
    Case("r2_n9216", R3[:2], 9216, "fused backward, odd number of 1024-blocks", fast="FF", bwd="own+fused"),
    Case("r2_2048_first_n9216", (R2K, R5C), 9216, "fused backward with 2048 listed first: the pair trades places", fast="FF", bwd="own+fused"),
    # ---- single fast resolutions ----------------------------------------------------------------------------------------------------
    Case("r512_n1024", R3[:1], 1024, "shortest row of the 512-point fast kernels: one backward strip", fast="F", bwd="own"),
    Case("r512_n1280", R3[:1], 1280, "5 hops: one strip of 5 blocks", fast="F", bwd="own"),
    Case("r2048_n4096", R3[1:2], 4096, "2048 alone owns the gradient buffer", fast="F", bwd="own"),
    Case("r8192_n20480", R3[2:], 20480, "8192 alone: seams added atomically onto a zeroed buffer", fast="F", bwd="zero"),
    Case("r2048_r8192_n16384", (R2K, R8), 16384, "seam hand-over picked up by a stand-alone 2048 launch", fast="FF", bwd="seam"),
    Case("r512_r8192_n16384", (R5C, R8), 16384, "seam hand-over picked up by a stand-alone 512 launch", fast="FF", bwd="seam"),
    # ---- all three fast: single-launch forward, seam hand-over into the fused launch --------------------------------------------------
    Case("r3_rows1x1_n16384", R3, 16384, "one row of the shortest all-fast length", rows=(1, 1), fast="FFF", bwd="seam+fused"),
    Case("r3_rows3x1_n20480", R3, 20480, "odd row count in the single-launch forward (rows are paired / grouped by 8 there)",
         rows=(3, 1), fast="FFF", bwd="seam+fused"),
    Case("r3_rows5x1_n28672", R3, 28672, "odd row count, 7 blocks of 4096", rows=(5, 1), fast="FFF", bwd="seam+fused"),
    Case("r3_global_sc_rows3x1_n16384", R3, 16384, "batch-global spectral convergence on the fast kernels", rows=(3, 1),
         kw=GLOBAL_SC, fast="FFF", bwd="seam+fused"),
    Case("r3_rows129x2_n16384", R3, 16384, "258 rows: above the 8192-point backward's 256 resident slots, strips laid out anew",
         rows=(129, 2), fast="FFF", bwd="seam+fused", sim="never"),
    # ---- mixtures and duplicates ----------------------------------------------------------------------------------------------------
    Case("r3_plus_1024_128_n16384", R3 + ((1024, 256, 1024), (128, 64, 128)), 16384,
         "five resolutions: three fast forwards launched one by one, two generic; backward all generic", rows=(1, 1), fast="FFFgg"),
    Case("dup512_r2048_n4096", (R5C, R5C, R2K), 4096, "512 listed twice: no fused launch, three owner-computes launches",
         fast="FFF", bwd="own"),
    Case("dup8192_n16384", (R8, R8), 16384, "8192 listed twice: only the first takes the fast kernels (two seam-mode launches "
         "would overwrite each other), so the backward is all generic", fast="Fg"),
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def qualifies(nf, hop, win, n):
    """the shape of resolution and row the register-radix kernels are written for"""
    return nf in (512, 2048, 8192) and 2 * hop == nf and win == nf and n >= 2 * nf and n % hop == 0


def route_by_rule(case):
    """(fast, bwd) as the rules in the module docstring give them"""
    fast, seen_8192 = [], False
    for nf, hop, win in case.res:
        f = qualifies(nf, hop, win, case.n) and not (nf == 8192 and seen_8192)
        seen_8192 = seen_8192 or (f and nf == 8192)
        fast.append(f)
    if not all(fast):
        return tuple(fast), "generic"
    sizes = [r[0] for r in case.res]
    n8, halo = sizes.count(8192), len(sizes) - sizes.count(8192)
    bwd = "own" if n8 == 0 else ("seam" if halo else "zero")
    if sizes.count(512) == 1 and sizes.count(2048) == 1 and case.n % 1024 == 0 and case.n >= 8192:
        bwd += "+fused"
    return tuple(fast), bwd


def _up(v):
    return (v + 63) // 64 * 64


def workspace_floats(case):
    """The plan's workspace (make_plan, mst_stft.hip) for the route the case states: partial sums | row sums | two coefficient blocks |
    tickets | the seam slab ("seam" routes) | per FAST resolution the kept target magnitudes and prediction spectra.  The strip lengths
    (3 / 6 / 5 frames per forward workgroup of the fast kernels) are the build's defaults."""
    rows, n, part = case.n_rows, case.n, 0
    for (nf, hop, _), fast in zip(case.res, case.fast_flags):
        frames = 1 + n // hop
        if fast:
            groups = max(frames // {512: 3, 2048: 6, 8192: 5}[nf], 1)
        else:
            groups = (frames + 1) // 2 if frames * rows >= 1024 else frames
        part += rows * groups * 4
    total = _up(part) + 3 * _up(len(case.res) * rows * 4) + 64
    if case.bwd.startswith("seam"):
        total += _up(rows * n)
    for (nf, hop, _), fast in zip(case.res, case.fast_flags):
        if fast:
            plane = rows * (1 + n // hop) * (nf // 2 + 1)
            total += _up(plane) + _up(2 * plane)
    return total


def draw(case):
    torch.manual_seed(case.seed)
    x = 0.3 * torch.randn(*case.rows, case.n)
    y = 0.5 * x + 0.2 * torch.randn(*case.rows, case.n)
    return x, y


def oracle(x, y, res, kw, dtype):
    """(loss, gradient) of oracle.loss_restated.mrstft_loss evaluated in `dtype`"""
    from oracle import loss_restated as ol

    xo = x.detach().cpu().to(dtype).requires_grad_(True)
    lo = ol.mrstft_loss(xo, y.detach().cpu().to(dtype), res, **kw)
    lo.backward()
    return lo.item(), xo.grad.double()


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """Inputs and both oracles of a case: computed once per session, shared by every test that grades the case, never modified."""
    case = BY_ID[case_id]
    x, y = draw(case)
    l64, g64 = oracle(x, y, case.res, case.kw, torch.float64)
    l32, g32 = oracle(x, y, case.res, case.kw, torch.float32)
    return dict(x=x, y=y, l64=l64, g64=g64, l32=l32, g32=g32)


def unreached(case):
    """bool (n,): samples no frame touches, reflect padding folded back (all False unless hop >= n_fft)"""
    n = case.n
    hit = torch.zeros(n, dtype=torch.bool)
    for nf, hop, _ in case.res:
        idx = (torch.arange(1 + n // hop)[:, None] * hop + torch.arange(nf)[None, :] - nf // 2).reshape(-1)
        idx = torch.where(idx < 0, -idx, idx)
        idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx)
        hit[idx] = True
    return ~hit


def grade(case, loss, grad, record=None, scale=1.0, ref=None, what=""):
    """Holds `loss` (a float) and `grad` (a tensor shaped like the prediction) of a HIP evaluation of `scale` x the case's loss against
    the bounds of the module docstring; files the measured figures through `record`."""
    ref = ref or reference(case.id)
    g = grad.detach().cpu().double().reshape(ref["g64"].shape)
    assert not torch.isnan(g).any(), f"{int(torch.isnan(g).sum())} gradient samples were never written"
    assert torch.isfinite(g).all() and loss == loss
    g64, g32, l64 = scale * ref["g64"], scale * ref["g32"], ref["l64"]
    e_loss = abs(loss - l64) / l64
    norm, peak = g64.norm().item(), g64.abs().max().item()
    h, r = (g - g64).norm().item() / norm, (g32 - g64).norm().item() / norm
    hp, rp = (g - g64).abs().max().item() / peak, (g32 - g64).abs().max().item() / peak
    print(f"\n[mrstft route {case.id}{what}: fast {case.fast or '-'} bwd {case.bwd}] loss {e_loss:.2e}; gradient rel-L2 HIP {h:.2e} "
          f"fp32 oracle {r:.2e}; per sample / peak HIP {hp:.2e} fp32 oracle {rp:.2e}")
    if record is not None:
        record(loss=e_loss, grad=(h, r), grad_per_sample=(hp, rp))
    assert e_loss < 1e-5, (loss, l64)
    assert h <= 2 * r + 1e-5, (h, r)
    assert hp <= 2 * rp + 1e-5, (hp, rp)
    gap = unreached(case)
    if gap.any():
        assert float(g[..., gap].abs().max()) == 0.0, "a sample no frame reaches has a gradient"
    return h, r
