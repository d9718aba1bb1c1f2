"""The encoder's 3x3 convolutions one at a time, on every kernel the launchers can choose: the case table, the dispatch rules restated,
the input recipe and the grading shared by tests/test_conv_routes_cpu.py and tests/test_conv_routes_gpu.py.  A plain module, no conftest.

The seam is the C ABI's mst_conv3x3 / mst_conv_wgrad (include/diffmst_hip.h): for ONE layer the weight preparation, the launcher and
the fold the network runs for it.  Which kernel runs is decided by workgroup counts (diff-mst_amd/csrc/mst_cnn.hip launch_conv3x3,
conv_csplit, conv_wgrad_nine_taps, launch_conv_wgrad; mst_cnn_net.hip wgrad_part_floats); `route_by_rule` restates those rules, every
case states the route it means to hit, and the CPU test holds the two against each other and against REACHABLE.

Image convention (mst_cnn.h, diffmst_hip/panns.py Cnn14.forward: x (bs, 1, bins, frames) -> x.reshape(bs, bins, frames).transpose(1, 2)):
the kernels' NHWC image has H = frames, W = bins, torch's NCHW image has H = bins, W = frames; weights stay in torch's layout.  So
torch_image = kernel_image.permute(0, 3, 2, 1) and back by the same permutation; nothing else of the kernels is restated here.

Exactness.  Activations and cotangents are integers in [-3, 3], weights integers in [-8, 8] without 0: every operand is a bf16 value, the
low pieces of the bf16x3 / bf16x6 splits are zero, every product and every partial sum is an integer, and max sum |x| |w| = 24 x 9 x 2048
< 2^24 (weight gradient: 9 P <= 2^24 for every P of the table), so fp32 accumulation is exact in ANY order - on the matrix pipe, across
split-K slabs, across pixel splits.  All four precisions must give the float64 reference bit for bit (bf16 storage: its round-to-nearest
-even bf16).  One wrong element anywhere fails; no tolerance is involved.

Statistics (`grade_stats`).  part[tile][c] = (sum v, sum v^2) over the tile's pixels of the fp32 results v, each an fp32 accumulation of
at most 256 terms (k_conv_igemm / 3: 4 per lane, 4 shuffle levels, 1 add = 128 pixels; k_conv_igemm4: 8 + 4 + 1 for 256 pixels;
k_conv_splitk_reduce: 4 per lane then 32 in sequence; k_conv1: 64 per lane, 3 levels, 2 adds for 2048 pixels - never more than 255
additions behind any term).  An fp32 sum of n terms s_n carries |s_n - sum v| <= (n - 1) 2^-24 sum |v| to first order, so per channel,
with the tiles folded in float64,  |sum_part - sum_ref| <= 256 x 2^-24 x sum |v|  and likewise for v^2 (v v is formed inside an fma,
unrounded).  The references are the float64 sums of the exact integer outputs.

Low pieces (`PIECE_CASES`).  Integer operands leave the low pieces of bf16x3 / bf16x6 zero and cannot see a dropped or mispaired cross term
of mma_split.  There the left operand has ONE non-zero element per result (a full-mantissa fp32 value), the right operand is dense
N(0, 1) fp32: every result is one product a b and the accumulation adds exact zeros.  `split_pieces` splits both operands as split8 does
(hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even; x3 keeps hi and lo = bf16(x - hi)); the reference is the
float64 sum of the terms mma_split<TERMS> keeps (3: lo hi, hi lo, hi hi; 6: lo hi, hi lo, mid mid, mid hi, hi mid, hi hi), every one a
product of two bf16 values, exact in fp32.  The kernel adds them one matrix instruction at a time onto an fp32 accumulator: at most TERMS
roundings, |out - ref| <= TERMS x 2^-24 x sum |kept terms|.  Precision 1 (fp32 operands) is the control with one term, a b itself.
"""
import functools
import zlib
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

PRECISIONS = {0: "bf16", 1: "fp32", 2: "bf16x3", 3: "bf16x6"}
CHANNELS = (64, 128, 256, 512, 1024, 2048)
X_MAX, W_MAX = 3, 8  # integer operand ranges
CONV_PIX, FAT_PIX, CONV1_PIX, WGRAD_PIX = 128, 256, 2048, 32
FAT_MIN = 1024  # MST_CONV_FAT_MIN
WGRAD4_WGS = 512  # MST_WGRAD4_WGS


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Route:
    kernel: str
    tiles: int = 0      # conv: pixel tiles whose statistics are written
    csplit: int = 0     # conv: 0 = unsplit, else 9 csplit slabs folded by k_conv_splitk_reduce
    splits: int = 0     # wgrad: pixel splits
    steps: int = 0      # wgrad: K steps (32 pixels) per split


@dataclass(frozen=True)
class Case:
    tag: str            # operands and direction; the id adds the precision
    shape: tuple        # (N, H, W, Cin, Cout): Cin / Cout are the WEIGHT's, whatever the direction
    precision: int
    direction: str      # "fwd" | "dgrad" | "wgrad"
    route: str          # the kernel the case means to hit ("+splitK<csplit>" when the K split runs)
    why: str
    scratch: bool = False   # conv: split-K scratch is passed
    split: tuple = ()       # wgrad: the (splits, steps_per_split) the case means to get

    @property
    def id(self):
        return f"{self.tag}-{PRECISIONS[self.precision]}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) & 0xFFFFFFFF

    @property
    def pixels(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def gemm(self):
        """(K channels, result channels) of the launch: swapped for the data gradient"""
        _, _, _, cin, cout = self.shape
        return (cout, cin) if self.direction == "dgrad" else (cin, cout)

    @property
    def storage(self):
        return torch.bfloat16 if self.precision == 0 else torch.float32


# ---- the dispatch rules ----------------------------------------------------------------------------------------------------------------
def conv_csplit(pixels, kin, kout):
    """conv_csplit: layers of fewer than 512 workgroups split K = 9 kin over 9 csplit workgroups"""
    bc = 128 if kout % 128 == 0 else 64
    wgs = cdiv(pixels, CONV_PIX) * (kout // bc)
    if wgs >= 512:
        return 0
    cs = 1
    while wgs * 9 * cs < 1024 and kin // (cs * 2) >= 128:
        cs *= 2
    return cs


def splitk_bytes(pixels, kin, kout):
    return 9 * conv_csplit(pixels, kin, kout) * pixels * kout * 4


def conv_route(precision, pixels, kin, kout, scratch):
    """launch_conv3x3, branch for branch (k_conv1 when kin == 1: cnn_forward_t)"""
    ty = "bf16" if precision == 0 else "float"
    if kin == 1:
        return Route(f"k_conv1<{ty}>", tiles=cdiv(pixels, CONV1_PIX))
    cs = conv_csplit(pixels, kin, kout) if scratch else 0
    bc = 128 if kout % 128 == 0 else 64
    tiles, tiles2 = cdiv(pixels, CONV_PIX), cdiv(pixels, FAT_PIX)
    fat_ok = precision == 0 and not cs and kout % 128 == 0 and tiles2 * (kout // 128) >= FAT_MIN
    if precision == 0 and not cs and tiles2 * (kout // bc) >= FAT_MIN:
        return Route(f"k_conv_igemm4<{bc},256>", tiles=tiles2)
    if fat_ok:  # never taken: kout % 128 == 0 makes bc 128 and the condition above the same inequality
        return Route("k_conv_igemm3<128,256>", tiles=tiles2)
    kernel = f"k_conv_igemm3<{bc},128>" if precision == 0 else f"k_conv_igemm<float,{bc}>"
    return Route(kernel + (f"+splitK{cs}" if cs else ""), tiles=tiles, csplit=cs)


def wgrad_nine_taps(precision, w, cin, cout):
    return precision == 0 and w >= 64 and cin % 64 == 0 and cout % 64 == 0


def wgrad_route(precision, n, h, w, cin, cout):
    """launch_conv_wgrad's kernel and wgrad_part_floats' split: about 2048 workgroups, at least 8 K steps per split"""
    pixels = n * h * w
    ksteps = cdiv(pixels, WGRAD_PIX)
    ty = "bf16" if precision == 0 else "float"
    if wgrad_nine_taps(precision, w, cin, cout):
        kernel, tiles = "k_conv_wgrad4", (2048 // WGRAD4_WGS) * (cout // 64) * (cin // 64)
    elif cin == 1:
        kernel, tiles = f"k_conv_wgrad<{ty},first>", 1
    elif cin % 128 == 0 and cout % 128 == 0:
        kernel, tiles = ("k_conv_wgrad3<128,128>" if precision == 0 else "k_conv_wgrad<float,128,128>"), (cout // 128) * (cin // 128) * 9
    else:
        kernel, tiles = ("k_conv_wgrad3<64,64>" if precision == 0 else "k_conv_wgrad<float,64,64>"), (cout // 64) * (cin // 64) * 9
    s = max(min(cdiv(2048, tiles), cdiv(ksteps, 8)), 1)
    per = cdiv(ksteps, s)
    return Route(kernel, splits=cdiv(ksteps, per), steps=per)


def wgrad_floats(route, cin, cout):
    return route.splits * (cout * 16 if cin == 1 else 9 * cout * cin)


def route_by_rule(case):
    n, h, w, cin, cout = case.shape
    if case.direction == "wgrad":
        return wgrad_route(case.precision, n, h, w, cin, cout)
    kin, kout = case.gemm
    return conv_route(case.precision, case.pixels, kin, kout, case.scratch)


def rounded_grid(route):
    """k_conv_wgrad3 / 4 decode a 1-D grid whose split count is rounded up to the 8 XCDs: workgroups past `splits` must leave at once"""
    return cdiv(route.splits, 8) * 8 if route.kernel.startswith(("k_conv_wgrad3", "k_conv_wgrad4")) else route.splits


def wgrad_traits(case):
    """which of the awkward properties a weight-gradient case has"""
    r = route_by_rule(case)
    ksteps = cdiv(case.pixels, WGRAD_PIX)
    return dict(ragged=case.pixels % WGRAD_PIX != 0, idle=r.splits % 8 != 0, short_last=ksteps - (r.splits - 1) * r.steps < r.steps and r.splits > 1)


# every (kernel, precision, direction) the rules can produce for Cnn14's channel counts; the CPU test derives the same set by enumeration
def _reachable():
    out = set()
    for p in PRECISIONS:
        ty = "bf16" if p == 0 else "float"
        out.add((f"k_conv1<{ty}>", p, "fwd"))
        out.add((f"k_conv_wgrad<{ty},first>", p, "wgrad"))
        for d in ("fwd", "dgrad"):
            for bc in (64, 128):
                base = f"k_conv_igemm3<{bc},128>" if p == 0 else f"k_conv_igemm<float,{bc}>"
                out.add((base, p, d))
                out.add((base + "+splitK", p, d))
                if p == 0:
                    out.add((f"k_conv_igemm4<{bc},256>", p, d))
        if p == 0:
            out |= {("k_conv_wgrad4", p, "wgrad"), ("k_conv_wgrad3<128,128>", p, "wgrad"), ("k_conv_wgrad3<64,64>", p, "wgrad")}
        else:
            out |= {("k_conv_wgrad<float,128,128>", p, "wgrad"), ("k_conv_wgrad<float,64,64>", p, "wgrad")}
    return frozenset(out)


REACHABLE = _reachable()


def route_key(kernel, precision, direction):
    """a route as REACHABLE names it: the csplit value dropped"""
    return (kernel.split("+splitK")[0] + ("+splitK" if "+splitK" in kernel else ""), precision, direction)


# ---- the table -------------------------------------------------------------------------------------------------------------------------
ALL, F32 = (0, 1, 2, 3), (1, 2, 3)


def _igemm(bc, cs=0):
    """the implicit-GEMM kernel of every precision for a channel tile (and a K split)"""
    sfx = f"+splitK{cs}" if cs else ""
    f32 = f"k_conv_igemm<float,{bc}>{sfx}"
    return {0: f"k_conv_igemm3<{bc},128>{sfx}", 1: f32, 2: f32, 3: f32}


def _conv(tag, shape, routes, why, dirs=("fwd", "dgrad"), precisions=ALL, scratch=False):
    """the cases of one shape; routes: {precision: kernel}, or one such dict per direction"""
    out = []
    for i, d in enumerate(dirs):
        r = routes[i] if isinstance(routes, tuple) else routes
        out += [Case(f"{d}-{tag}" + ("-scratch" if scratch else ""), shape, p, d, r[p], why, scratch=scratch) for p in precisions]
    return out


def _wgrad(tag, shape, kernels, split, why, precisions=ALL):
    return [Case(f"wgrad-{tag}", shape, p, "wgrad", kernels[p], why, split=split) for p in precisions]


_F128, _F64 = "k_conv_wgrad<float,128,128>", "k_conv_wgrad<float,64,64>"
_WG128 = {0: "k_conv_wgrad3<128,128>", 1: _F128, 2: _F128, 3: _F128}
_WG64 = {0: "k_conv_wgrad3<64,64>", 1: _F64, 2: _F64, 3: _F64}
_WG4_64 = {0: "k_conv_wgrad4", 1: _F64, 2: _F64, 3: _F64}     # W >= 64: bf16 runs all nine taps in one workgroup
_WG4_128 = {0: "k_conv_wgrad4", 1: _F128, 2: _F128, 3: _F128}
_WG1 = {0: "k_conv_wgrad<bf16,first>", 1: "k_conv_wgrad<float,first>", 2: "k_conv_wgrad<float,first>", 3: "k_conv_wgrad<float,first>"}
_C1 = {0: "k_conv1<bf16>", 1: "k_conv1<float>", 2: "k_conv1<float>", 3: "k_conv1<float>"}

CASES = tuple(
    # ---- unsplit (no scratch): k_conv_igemm (fp32 / x3 / x6) and k_conv_igemm3<BC, 128> (bf16) ------------------------------------------
    _conv("n2h5w13-c64-c64", (2, 5, 13, 64, 64), _igemm(64), "P = 130: one full tile and two pixels; the full tile straddles the two images")
    + _conv("n3h7w33-c128-c128", (3, 7, 33, 128, 128), _igemm(128), "P = 693, three images, odd width: tiles 1, 3 straddle image boundaries")
    + _conv("n3h5w13-c64-c128", (3, 5, 13, 64, 128), (_igemm(128), _igemm(64)), "Cin 64 -> Cout 128: the two directions take different channel tiles")
    + _conv("n2h7w33-c128-c64", (2, 7, 33, 128, 64), (_igemm(64), _igemm(128)), "Cin 128 -> Cout 64, P = 462")
    # ---- degenerate widths: every pixel is an edge, fewer pixels than a tile -------------------------------------------------------------
    + _conv("n1h4w2-c1024", (1, 4, 2, 1024, 1024), _igemm(128), "last blocks: W = 2, every pixel on the left or the right edge")
    + _conv("n2h2w1-c2048", (2, 2, 1, 2048, 2048), _igemm(128), "W = 1: no horizontal neighbour exists at all")
    + _conv("n3h1w2-c1024", (3, 1, 2, 1024, 1024), _igemm(128), "H = 1: no vertical neighbour; three images of two pixels in one tile")
    + _conv("n2h1w1-c2048", (2, 1, 1, 2048, 2048), _igemm(128), "1 x 1 images: only the centre tap is ever inside")
    # ---- split K (scratch passed), folded by k_conv_splitk_reduce ---------------------------------------------------------------------
    + _conv("n2h5w13-c64-c64", (2, 5, 13, 64, 64), _igemm(64, 1), "nine tap workgroups per tile (csplit 1), 64-channel tile; P = 130", scratch=True)
    + _conv("n3h7w33-c256-c512", (3, 7, 33, 256, 512), (_igemm(128, 2), _igemm(128, 4)),
            "forward K 256 / 2, data gradient K 512 / 4 (channel roles swapped); P = 693", scratch=True)
    + _conv("n1h9w21-c512-c256", (1, 9, 21, 512, 256), (_igemm(128, 4), _igemm(128, 2)),
            "few workgroups: forward K 512 / 4, data gradient K 256 / 2; P = 189", scratch=True)
    + _conv("n1h4w2-c2048", (1, 4, 2, 2048, 2048), _igemm(128, 8), "csplit 8 on one ragged tile of 8 pixels, W = 2", scratch=True)
    + _conv("n2h2w1-c1024-c2048", (2, 2, 1, 1024, 2048), (_igemm(128, 8), _igemm(128, 16)),
            "the largest csplit the rule yields (K 2048 into 8 result-channel tiles: 16) on W = 1", scratch=True)
    + _conv("n2h1w1-c1024", (2, 1, 1, 1024, 1024), _igemm(128, 8), "1 x 1 images through the K split: eight of nine tap slabs are all zero", scratch=True)
    # ---- 512 workgroups and more: never split, scratch or not ----------------------------------------------------------------------------
    + _conv("n1h64w1023-c64-c64", (1, 64, 1023, 64, 64), _igemm(64), "512 workgroups (P = 65 472, last tile ragged): the scratch that is passed stays unused",
            precisions=F32, scratch=True)
    # ---- k_conv_igemm4 (bf16, 256-pixel tiles): from tiles2 x (Cout / bc) = 1024 workgroups --------------------------------------------
    + _conv("n1h257w1021-c64-c64", (1, 257, 1021, 64, 64), {0: "k_conv_igemm4<64,256>"},
            "smallest odd-width image of 1024 fat tiles and more: P = 262 397 = 1024 x 256 + 253", precisions=(0,))
    + _conv("n1h257w1021-c64-c128", (1, 257, 1021, 64, 128), {0: "k_conv_igemm4<128,256>"},
            "128-channel fat tile; Cout / bc = 1 for both tiles, so 128 channels need the same 1024 pixel tiles as 64", dirs=("fwd",), precisions=(0,))
    + _conv("n1h257w1021-c128-c64", (1, 257, 1021, 128, 64), {0: "k_conv_igemm4<128,256>"},
            "the 128-channel fat tile on the data-gradient weights", dirs=("dgrad",), precisions=(0,))
    # ---- first layer -----------------------------------------------------------------------------------------------------------------
    + _conv("n2h5w411-c1-c64", (2, 5, 411, 1, 64), _C1, "k_conv1: P = 4110 = 2 x 2048 + 14, odd width, the image boundary inside tile 1", dirs=("fwd",))
    # ---- weight gradient: (splits, steps_per_split) as wgrad_part_floats cuts the pixels ------------------------------------------------
    + _wgrad("n1h11w64-c64-c64", (1, 11, 64, 64, 64), _WG4_64, (3, 8), "W = 64: the nine-tap kernel's smallest width; 22 K steps as 8 + 8 + 6")
    + _wgrad("n1h9w65-c64-c64", (1, 9, 65, 64, 64), _WG4_64, (3, 7), "W = 65: the row end moves through the stages; P = 585 = 18 x 32 + 9, splits 7 + 7 + 5")
    + _wgrad("n1h13w129-c128-c128", (1, 13, 129, 128, 128), _WG4_128, (7, 8), "W = 129, 2 x 2 channel tiles of the nine-tap kernel; 53 K steps, last split 5")
    + _wgrad("n2h9w65-c64-c128", (2, 9, 65, 64, 128), _WG4_64, (5, 8), "two images, Cin 64 -> Cout 128 (64-channel tiles for every precision)")
    + _wgrad("n3h7w33-c128-c128", (3, 7, 33, 128, 128), _WG128, (3, 8), "W < 64: one tap per workgroup; P = 693, splits 8 + 8 + 6, five idle workgroups per tile")
    + _wgrad("n3h7w33-c64-c128", (3, 7, 33, 64, 128), _WG64, (3, 8), "the 64-channel tiles on the same pixels")
    + _wgrad("n3h199w1-c64-c64", (3, 199, 1, 64, 64), _WG64, (3, 7), "W = 1 over three splits: the horizontal taps never see a pixel")
    + _wgrad("n1h4w2-c1024", (1, 4, 2, 1024, 1024), _WG128, (1, 1), "last blocks: 8 pixels of W = 2, one ragged K step")
    + _wgrad("n2h2w1-c2048", (2, 2, 1, 2048, 2048), _WG128, (1, 1), "4 pixels of W = 1 at 2048 channels")
    + _wgrad("n1h9w65-c1-c64", (1, 9, 65, 1, 64), _WG1, (3, 7), "first layer: the taps of the fp32 spectrogram as the B operand; splits 7 + 7 + 5")
    + _wgrad("n2h5w411-c1-c64", (2, 5, 411, 1, 64), _WG1, (17, 8), "first layer, 17 splits (k_wgrad_reduce_first folds 16 at a time), last split one step")
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
STATS_CASES = tuple(c for c in CASES if c.direction == "fwd")  # the network asks for statistics in the forward only


# ---- operands and references -----------------------------------------------------------------------------------------------------------
def to_torch_image(x):
    """kernel image (N, H = frames, W = bins, C) <-> torch image (N, C, bins, frames): the same permutation both ways"""
    return x.permute(0, 3, 2, 1)


def _ints(g, shape, bound, zero=True):
    v = torch.randint(-bound, bound + 1, shape, generator=g)
    if not zero:  # dense: every (tap, channel) slot of every filter carries a value
        v = torch.where(v == 0, torch.randint(1, bound + 1, shape, generator=g), v)
    return v.to(torch.float32)


def draw(case):
    """the operands of a case as fp32 CPU tensors in the ABI's layouts: x / dy NHWC (first layer: x (N, H, W)), w (Cout, Cin, 3, 3)"""
    g = torch.Generator().manual_seed(case.seed)
    n, h, w, cin, cout = case.shape
    ops = {}
    if case.direction in ("fwd", "wgrad"):
        ops["x"] = _ints(g, (n, h, w) if cin == 1 else (n, h, w, cin), X_MAX)
    if case.direction in ("dgrad", "wgrad"):
        ops["dy"] = _ints(g, (n, h, w, cout), X_MAX)
    if case.direction != "wgrad":
        ops["w"] = _ints(g, (cout, cin, 3, 3), W_MAX, zero=False)
    return ops


def magnitude_bound(case, ops):
    """max over the results of sum |a| |b|: every partial sum of the kernel, in any order, is an integer no larger than this"""
    return float(reference_of(case, {k: v.abs() for k, v in ops.items()}).max())


def reference_of(case, ops):
    """float64 torch.nn.functional.conv2d (or its gradients) on the torch layouts, back in the ABI's layout"""
    n, h, w, cin, cout = case.shape
    d = {k: v.double() for k, v in ops.items()}
    if "x" in d:
        xt = to_torch_image(d["x"].reshape(n, h, w, cin))
    if "dy" in d:
        gt = to_torch_image(d["dy"])
    if case.direction == "fwd":
        return to_torch_image(F.conv2d(xt, d["w"], None, stride=1, padding=1)).contiguous()
    if case.direction == "dgrad":
        return to_torch_image(torch.nn.grad.conv2d_input((n, cin, w, h), d["w"], gt, stride=1, padding=1)).contiguous()
    return torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), gt, stride=1, padding=1).contiguous()


@functools.lru_cache(maxsize=4)
def reference(case_id):
    """operands and float64 reference of a case: computed once, never modified.  Only the last few stay (the largest is 270 MB)."""
    case = BY_ID[case_id]
    ops = draw(case)
    return dict(ops=ops, ref=reference_of(case, ops))


@functools.lru_cache(maxsize=None)
def channel_sums(case_id):
    """per channel of a convolution's exact output v: (sum v, sum |v|, sum v^2) in float64 - what the statistics are graded against; kept
    for the whole session, so that the statistics test does not form the reference a second time"""
    ref = reference(case_id)["ref"]
    v = ref.reshape(-1, ref.shape[-1])
    return v.sum(0), v.abs().sum(0), (v * v).sum(0)


def device_bytes(case):
    """what a case holds on the device: operands, result, statistics, prepared weights, split-K slabs / partial weight gradients"""
    n, h, w, cin, cout = case.shape
    P, esz = case.pixels, (2 if case.precision == 0 else 4)
    if case.direction == "wgrad":
        return P * cout * esz + P * cin * (4 if cin == 1 else esz) + 9 * cin * cout * 4 + 4 * wgrad_floats(route_by_rule(case), cin, cout)
    kin, kout = case.gemm
    total = P * kin * (4 if cin == 1 else esz) + P * kout * esz + 9 * cin * cout * 4 + 2 * 9 * cin * cout * esz
    total += cdiv(P, CONV_PIX) * kout * 2 * 4
    return total + (splitk_bytes(P, kin, kout) if case.scratch else 0)


LARGEST = ("fwd-n1h4w2-c2048-scratch-fp32", 457_850_880)  # bytes: 2048 x 2048 x 9 weights as given and in both operand layouts, 3 x 151 MB


# ---- grading ---------------------------------------------------------------------------------------------------------------------------
def first_difference(out, want):
    """(count, coordinates of the first differing element); NaN (an element no kernel wrote) differs from everything"""
    bad = ~(out == want)
    count = int(bad.sum())
    return count, (tuple(int(i) for i in bad.nonzero()[0]) if count else None)


def grade_exact(case, out, ref):
    """out: the kernel's result on the host in its storage type; ref: the float64 reference.  Bit for bit."""
    want = ref.to(torch.float32)
    assert torch.equal(want.double(), ref) and torch.equal(ref, ref.round()), "the reference is not an integer that fp32 holds"
    if out.dtype == torch.bfloat16:
        want = want.to(torch.bfloat16)
    assert out.shape == want.shape and out.dtype == want.dtype
    count, at = first_difference(out, want)
    names = "(co, ci, kh, kw)" if case.direction == "wgrad" else "(n, h, w, c)"
    assert count == 0, (f"{case.id} [{case.route}]: {count} of {out.numel()} elements differ, first at {names} = {at}: "
                        f"got {out[at].item()!r}, expected {want[at].item()!r}")


def grade_stats(case, part, tiles, sums):
    """part (>= tiles, C, 2) fp32 on the host, sums = channel_sums(case.id): the module docstring's bound, per channel.  Returns the two
    largest errors as fractions of their bounds."""
    s1, a1, s2 = sums
    p = part[:tiles].double()
    assert p.shape == (tiles, s1.numel(), 2)
    assert not torch.isnan(p).any(), f"{int(torch.isnan(p).any(-1).sum())} (tile, channel) statistics were never written"
    got, used = p.sum(0), []
    for k, (name, want, mag) in enumerate((("sum", s1, a1), ("sum of squares", s2, s2))):
        err, bound = (got[:, k] - want).abs(), 256 * 2.0 ** -24 * mag
        worst = int((err - bound).argmax())
        assert (err <= bound).all(), (f"{case.id} [{case.route}]: {name} of channel {worst}: {got[worst, k].item()!r} vs "
                                      f"{want[worst].item()!r}, bound {bound[worst].item():.3e}")
        used.append(float((err / bound.clamp_min(1e-300)).max()))
    return tuple(used)


# ---- the low pieces --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PieceCase:
    shape: tuple        # (N, H, W, Cin, Cout)
    precision: int      # 1 (control), 2, 3
    direction: str

    @property
    def id(self):
        n, h, w, cin, cout = self.shape
        return f"{self.direction}-n{n}h{h}w{w}-c{cin}-c{cout}-{PRECISIONS[self.precision]}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode()) & 0xFFFFFFFF

    @property
    def terms(self):
        return {1: 1, 2: 3, 3: 6}[self.precision]


PIECE_CASES = tuple(PieceCase(s, p, d) for s in ((2, 5, 13, 64, 64), (1, 7, 19, 128, 128)) for d in ("fwd", "dgrad", "wgrad") for p in (1, 2, 3))


def bf16_round(x):
    """fp32 -> the fp32 value of its round-to-nearest-even bf16 (v_cvt_pk_bf16_f32, f2bf)"""
    return x.to(torch.bfloat16).to(torch.float32)


def split_pieces(x, terms):
    """the bf16 pieces of fp32 `x` as split8 forms them, as fp32 tensors: (hi, lo) for 3 terms, (hi, mid, lo) for 6"""
    assert x.dtype == torch.float32
    hi = bf16_round(x)
    r1 = x - hi  # exact: hi carries the leading 8 bits of x
    if terms == 3:
        return hi, bf16_round(r1)
    mid = bf16_round(r1)
    return hi, mid, bf16_round(r1 - mid)


def kept_terms(a, b, terms):
    """the products mma_split<terms> accumulates for a left-operand value a and a right-operand value b (fp32 tensors of one shape), in
    float64 (each is a product of two bf16 values: exact); terms = 1: the fp32 pipe's single product"""
    if terms == 1:
        return [a.double() * b.double()]
    pa, pb = [p.double() for p in split_pieces(a, terms)], [p.double() for p in split_pieces(b, terms)]
    if terms == 3:
        (ah, al), (bh, bl) = pa, pb
        return [al * bh, ah * bl, ah * bh]
    (ah, am, al), (bh, bm, bl) = pa, pb
    return [al * bh, ah * bl, am * bm, am * bh, ah * bm, ah * bh]


def _full_mantissa(g, shape):
    """fp32 values in +-[1, 2) with random low mantissa bits"""
    v = 1.0 + torch.rand(shape, generator=g, dtype=torch.float64)
    return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(torch.float32)


def draw_pieces(case):
    """Operands of a piece case and, per result element, the two factors of its single product.
    fwd   w has one non-zero (ci, kh, kw) per output channel co; x dense:           out[n, h, w, co] = w[co, ci, kh, kw] x[shifted pixel, ci]
    dgrad w has one non-zero (co, kh, kw) per INPUT channel ci; dy dense:           dx[n, h, w, ci] = w[co, ci, kh, kw] dy[shifted pixel, co]
    wgrad dy has one non-zero pixel per output channel co; x dense:                 gw[co, ci, kh, kw] = dy[pixel, co] x[shifted pixel, ci]
    The factor maps come from the float64 reference machinery itself (a conv of the one-hot operand with an all-ones partner selects the
    left factor, the full reference divided by it the product), so no tap arithmetic is restated: see `piece_factors`."""
    g = torch.Generator().manual_seed(case.seed)
    n, h, w, cin, cout = case.shape
    ops = {}
    if case.direction == "wgrad":
        dy = torch.zeros(n * h * w, cout)
        dy[torch.randint(0, n * h * w, (cout,), generator=g), torch.arange(cout)] = _full_mantissa(g, (cout,))
        ops["dy"], ops["x"] = dy.reshape(n, h, w, cout), torch.randn(n, h, w, cin, generator=g)
    else:
        rows = cout if case.direction == "fwd" else cin
        other = torch.randint(0, cin if case.direction == "fwd" else cout, (rows,), generator=g)
        kh, kw = torch.randint(0, 3, (rows,), generator=g), torch.randint(0, 3, (rows,), generator=g)
        wt = torch.zeros(cout, cin, 3, 3)
        if case.direction == "fwd":
            wt[torch.arange(rows), other, kh, kw] = _full_mantissa(g, (rows,))
            ops["x"] = torch.randn(n, h, w, cin, generator=g)
        else:
            wt[other, torch.arange(rows), kh, kw] = _full_mantissa(g, (rows,))
            ops["dy"] = torch.randn(n, h, w, cout, generator=g)
        ops["w"] = wt
    return ops


def piece_factors(case, ops):
    """(a, b): per result element the left-operand value and the right-operand value of its one product, fp32 exactly as the operands hold
    them; b = 0 where the partner pixel lies outside the image (a's choice is then irrelevant).  a comes from the reference convolution of
    the one-hot operand with an all-ones partner, b from the reference convolution of its 0/1 support with the dense partner - both are
    sums of one term, exact in float64 and in fp32."""
    left = "dy" if case.direction == "wgrad" else "w"
    right = "x" if case.direction in ("fwd", "wgrad") else "dy"
    ones = dict(ops)
    ones[right] = torch.ones_like(ops[right])
    a = reference_of(case, ones)  # the left value wherever the partner pixel exists, 0 at the image border
    support = dict(ops)
    support[left] = (ops[left] != 0).to(torch.float32)
    b = reference_of(case, support)
    af, bf = a.to(torch.float32), b.to(torch.float32)
    assert torch.equal(af.double(), a) and torch.equal(bf.double(), b)
    return af, bf


def grade_pieces(case, out, ops):
    """out: fp32 result on the host.  Returns (max |out - ref| / bound, max |out - a b| / |a b|); asserts the bound of the docstring."""
    a, b = piece_factors(case, ops)
    kept = kept_terms(a, b, case.terms)
    ref, mag = sum(kept), sum(t.abs() for t in kept)
    assert not torch.isnan(out).any(), "an element was never written"
    err, bound = (out.double() - ref).abs(), case.terms * 2.0 ** -24 * mag
    exact = a.double() * b.double()
    live = exact != 0
    assert int(live.sum()) * 2 > exact.numel(), "most results must carry a product"
    per_product = float(((out.double() - exact).abs()[live] / exact.abs()[live]).max())
    count = int((err > bound).sum())
    at = tuple(int(i) for i in np.unravel_index(int((err - bound).argmax()), tuple(err.shape))) if count else None
    assert count == 0, (f"{case.id}: {count} of {out.numel()} results leave the bound, worst at {at}: got {out[at].item()!r}, kept terms sum to "
                        f"{ref[at].item()!r}, a b = {exact[at].item()!r}, bound {bound[at].item():.3e}")
    return float((err / bound.clamp_min(1e-300))[live].max()), per_product


