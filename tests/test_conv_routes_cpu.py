"""The case table of tests/conv_routes.py held against the restated dispatch rules, without a GPU: every case takes the route it states,
every route the rules can produce is named by a case, the operands keep every partial sum exact, and the piece emulation is sound.  The
device side is tests/test_conv_routes_gpu.py."""
import itertools

import pytest
import torch

import conv_routes as cr


def test_every_case_takes_the_route_it_states():
    for c in cr.CASES:
        r = cr.route_by_rule(c)
        assert r.kernel == c.route, (c.id, c.route, r)
        if c.direction == "wgrad":
            assert (r.splits, r.steps) == c.split, (c.id, c.split, r)
        else:
            assert bool(r.csplit) == ("+splitK" in c.route) and (not r.csplit or c.scratch), c.id
        n, h, w, cin, cout = c.shape
        assert (cin in cr.CHANNELS and cout in cr.CHANNELS) or (cin, cout) == (1, 64), c.id  # Cnn14's channel counts
        assert c.why


def rules_over_the_shapes():
    """every (kernel, precision, direction) the rules give over Cnn14's channel pairs, a spread of pixel counts and widths, with and
    without scratch"""
    seen = set()
    pixel_counts = (1, 2, 8, 127, 128, 129, 693, 4110, 65408, 65409, 131072, 261888, 261889, 262397, 600000, 2 ** 22)
    for cin, cout in itertools.product((1,) + cr.CHANNELS, cr.CHANNELS):
        if cin == 1 and cout != 64:
            continue
        for p in cr.PRECISIONS:
            for pixels in pixel_counts:
                for scratch in (False, True):
                    seen.add(cr.route_key(cr.conv_route(p, pixels, cin, cout, scratch).kernel, p, "fwd"))
                    if cin > 1:
                        seen.add(cr.route_key(cr.conv_route(p, pixels, cout, cin, scratch).kernel, p, "dgrad"))
            for w in (1, 2, 33, 63, 64, 65, 129, 1025):
                for h in (1, 7, 64, 513):
                    seen.add((cr.wgrad_route(p, 2, h, w, cin, cout).kernel, p, "wgrad"))
    return seen


def test_the_rules_reach_exactly_the_reachable_routes():
    """REACHABLE is what the rules produce - in particular nothing reaches launch_conv3x3's `fat_ok` branch (k_conv_igemm3<128, 256>): its
    condition is the k_conv_igemm4 condition above it with Cout % 128 == 0 added."""
    seen = rules_over_the_shapes()
    assert seen == set(cr.REACHABLE), (sorted(seen - cr.REACHABLE), sorted(cr.REACHABLE - seen))
    assert not any(k.startswith("k_conv_igemm3<128,256>") for k, _, _ in seen)


def test_every_reachable_route_has_a_case():
    covered = {cr.route_key(c.route, c.precision, c.direction) for c in cr.CASES}
    assert covered == set(cr.REACHABLE), (sorted(cr.REACHABLE - covered), sorted(covered - cr.REACHABLE))
    # the K split: 1, 2, 4 and the largest value the rule yields for these channel counts, forward and data gradient
    largest = max(cr.conv_csplit(p, kin, kout) for p in (1, 2, 8, 128, 693) for kin in cr.CHANNELS for kout in cr.CHANNELS)
    assert largest == 16
    for d in ("fwd", "dgrad"):
        got = {cr.route_by_rule(c).csplit for c in cr.CASES if c.direction == d and c.scratch}
        assert {0, 1, 2, 4, 8} <= got and (d == "fwd" or largest in got), (d, got)
    # both storage types of k_conv_splitk_reduce on a pixel count that is no multiple of the tile
    for p in (0, 1):
        assert any(c.precision == p and "+splitK" in c.route and c.pixels % cr.CONV_PIX for c in cr.CASES)


def test_the_awkward_shapes_are_there():
    conv = [c for c in cr.CASES if c.direction != "wgrad"]
    assert all(c.pixels % cr.CONV_PIX for c in conv if "igemm<" in c.route or "igemm3" in c.route)
    assert all(c.pixels % cr.FAT_PIX for c in conv if "igemm4" in c.route)
    assert all(c.pixels % cr.CONV1_PIX and c.shape[2] % 2 for c in conv if "k_conv1" in c.route)
    assert any(c.shape[0] == 3 and c.pixels > cr.CONV_PIX and not c.scratch for c in conv)  # tiles that straddle image boundaries
    for hw in ((4, 2), (2, 1), (1, 2), (1, 1)):
        got = {c.shape[3] for c in conv if c.shape[1:3] == hw and c.shape[3] == c.shape[4] and not c.scratch}
        assert got & {1024, 2048}, hw
    # the 512-workgroup threshold from both sides, and the fat tile at the first pixel count that reaches it with this width
    assert cr.conv_csplit(65472 - 128, 64, 64) and not cr.conv_csplit(65472, 64, 64)
    assert cr.conv_route(0, 257 * 1021, 64, 64, False).kernel == "k_conv_igemm4<64,256>"
    assert cr.conv_route(0, 256 * 1021, 64, 64, False).kernel == "k_conv_igemm3<64,128>"
    # weight gradient: per kernel and precision a ragged last K step, a split count the 8-wide grid rounds up, a short last split
    wg = [c for c in cr.CASES if c.direction == "wgrad"]
    for key in {(c.route, c.precision) for c in wg}:
        traits = [cr.wgrad_traits(c) for c in wg if (c.route, c.precision) == key]
        for t in ("ragged", "idle", "short_last"):
            assert any(tr[t] for tr in traits), (key, t)
    assert {c.shape[2] for c in wg if c.route == "k_conv_wgrad4"} >= {64, 65, 129}
    assert {c.shape[2] for c in wg if c.route.startswith("k_conv_wgrad3")} >= {1, 2, 33}
    assert all(cr.rounded_grid(cr.route_by_rule(c)) > c.split[0] for c in wg if c.route.startswith(("k_conv_wgrad3", "k_conv_wgrad4")) and c.split[0] % 8)


def test_ids_and_seeds_are_distinct():
    assert len({c.seed for c in cr.CASES}) == len(cr.CASES)
    assert len({c.id for c in cr.PIECE_CASES}) == len(cr.PIECE_CASES)


# drawing 2048 x 2048 x 9 weights takes a second: the cases of 1024 channels and more are drawn here for two of their four precisions (the
# recipe does not look at the precision, only the seed differs); grade_exact asserts the integer reference of every case on the device run
DRAWN = [c for c in cr.CASES if max(c.shape[3:]) < 1024 or c.precision in (0, 1)]


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in DRAWN])
def test_operands_keep_the_accumulation_exact(case):
    """Dense integer operands inside their ranges (so bf16 values), an integer float64 reference that fp32 holds exactly, and - formed for
    the small cases, by the worst case of the shape for all of them in the next test - sum |a| |b| < 2^24 per result."""
    ops, ref = cr.reference(case.id)["ops"], cr.reference(case.id)["ref"]
    for name, v in ops.items():
        assert torch.equal(v, v.round()) and torch.equal(v.to(torch.bfloat16).float(), v)
        assert float(v.abs().max()) <= (cr.W_MAX if name == "w" else cr.X_MAX)
        assert float((v != 0).float().mean()) > 0.8  # dense
    if "w" in ops:
        assert bool((ops["w"] != 0).all())
    if case.pixels < 1000 and case.shape[3] * case.shape[4] <= 2 ** 17:
        assert cr.magnitude_bound(case, ops) < 2 ** 24
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    assert float(ref.abs().max()) > 0


def test_the_bound_holds_for_every_case_by_its_shape():
    """the large cases by the worst case of their shape: 9 K-channels (weight gradient: 9 P) products of at most X_MAX W_MAX (X_MAX^2)"""
    for c in cr.CASES:
        worst = 9 * c.pixels * cr.X_MAX ** 2 if c.direction == "wgrad" else 9 * c.gemm[0] * cr.X_MAX * cr.W_MAX
        assert worst < 2 ** 24, c.id


def test_device_memory_of_the_largest_case():
    big = max(cr.CASES, key=cr.device_bytes)
    assert (big.id, cr.device_bytes(big)) == cr.LARGEST
    assert cr.LARGEST[1] < 1e9


def test_six_pieces_reproduce_fp32_exactly():
    """hi + mid + lo = x for every fp32 x (24 significand bits in three bf16 pieces), two pieces leave at most 2^-16 |x|; a product's six
    kept terms miss a b by the dropped terms only: below 2^-22 |a b|, the three kept terms of bf16x3 by 2^-15 |a b|."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat((torch.randn(100000, generator=g), torch.randn(1000, generator=g) * 1e-6, torch.tensor([1.0, -1.0, 0.0, 1.9999999, 255.5, 1.0e38])))
    hi, mid, lo = cr.split_pieces(x, 6)
    for p in (hi, mid, lo):
        assert torch.equal(cr.bf16_round(p), p)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    h2, l2 = cr.split_pieces(x, 3)
    assert torch.equal(h2, hi) and torch.equal(l2, mid)
    assert bool(((x.double() - h2.double() - l2.double()).abs() <= 2.0 ** -16 * x.double().abs()).all())
    a, b = x[:50000], x[50000:100000]
    exact = a.double() * b.double()
    assert bool(((sum(cr.kept_terms(a, b, 6)) - exact).abs() <= 2.0 ** -22 * exact.abs()).all())
    assert bool(((sum(cr.kept_terms(a, b, 3)) - exact).abs() <= 2.0 ** -15 * exact.abs()).all())
    assert torch.equal(sum(cr.kept_terms(a, b, 1)), exact)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in cr.PIECE_CASES if c.precision == 3])
def test_piece_cases_are_single_products(case):
    """Every result of a piece case is ONE product of the factors `piece_factors` names: the float64 reference of the case equals a b."""
    ops = cr.draw_pieces(case)
    a, b = cr.piece_factors(case, ops)
    ref = cr.reference_of(case, ops)
    assert torch.equal(ref, a.double() * b.double())
    assert float((ref != 0).float().mean()) > 0.5
    # and grading the correctly rounded products as the fp32 pipe's output passes, a result with its low cross terms dropped does not
    one = cr.PieceCase(case.shape, 1, case.direction)
    cr.grade_pieces(one, ref.float(), ops)
    hi_only = cr.bf16_round(a).double() * cr.bf16_round(b).double()
    with pytest.raises(AssertionError):
        cr.grade_pieces(case, hi_only.float(), ops)


def test_the_host_simulator_has_the_entries_and_refuses_them():
    """The simulator library leaves the matrix-core kernels out; it still exports the whole ABI (the binding refuses a library that does
    not), with the encoder's answers for what it cannot run: 0 bytes and hipErrorNotSupported, before any pointer is looked at."""
    from hostsim import harness
    from mst import _cabi

    L = harness.lib()
    assert L.mst_conv3x3_workspace_bytes(1, 64, 64) == 0 and L.mst_conv3x3_splitk_bytes(2, 5, 13, 64, 64, 0) == 0
    assert L.mst_conv3x3_part_bytes(2, 5, 13, 64, 64, 0) == 0 and L.mst_conv_wgrad_workspace_bytes(1, 2, 5, 13, 64, 64) == 0
    with pytest.raises(_cabi.AbiError) as e:
        L.mst_conv3x3(1, 0, None, None, None, None, None, 2, 5, 13, 64, 64, None, 0, None, 0, None)
    assert e.value.code == 801
    with pytest.raises(_cabi.AbiError) as e:
        L.mst_conv_wgrad(1, None, None, None, 2, 5, 13, 64, 64, None, 0, None, None, None)
    assert e.value.code == 801
