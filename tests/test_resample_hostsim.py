"""The resampling kernels (diff-mst_amd/csrc/mst_resample.hip) on the host simulator, through the C ABI, against (1) the float64
restatement of torchaudio's algorithm (tests/resample_ref.py - parity with the package itself is UNPINNED, it is not installed),
(2) the integer output length, (3) a closed form that does not depend on the restatement, (4) the adjoint from autograd and the
dot-product identity, (5) determinism and batching, (6) edge cases.  tests/test_resample_gpu.py carries the same cases on the device."""
import pytest
import torch

import resample_ref as R
from resample_ref import RATIOS, RESTATEMENT_VS_CLOSED_FORM, SINE_RATIOS, case_lengths, check_forward, noise, sine_case

@pytest.fixture(scope="module")
def lib():
    from hostsim import harness

    return harness.lib()


_TABLES = {}


def tables(L, orig, new):
    if (orig, new) not in _TABLES:
        nbytes = L.mst_resample_tables_bytes(orig, new)
        assert nbytes > 0
        t = torch.zeros(nbytes // 4, dtype=torch.int32)
        L.mst_resample_init_tables(orig, new, t, None)
        _TABLES[(orig, new)] = t
    return _TABLES[(orig, new)]


GUARD = 64


def forward(L, x, orig, new):
    """x: float32 tensor (rows, n), unit sample stride, any row stride -> y (rows, n_out); the output buffer is pre-filled with
    NaN, must be overwritten completely and nothing may be written behind it."""
    rows, n = x.shape
    assert x.stride(1) == 1 or n == 1
    n_out = L.mst_resample_out_samples(n, orig, new)
    assert n_out == R.out_samples(n, orig, new)
    buf = torch.full((rows * n_out + GUARD,), float("nan"))
    L.mst_resample_forward(x, rows, n, x.stride(0), orig, new, tables(L, orig, new), buf, None)
    assert torch.isnan(buf[rows * n_out:]).all(), "written past the output"
    y = buf[: rows * n_out].view(rows, n_out)
    assert torch.isfinite(y).all(), "output not fully written"
    return y


def backward(L, g, n, orig, new):
    rows, n_out = g.shape
    assert g.is_contiguous() and n_out == R.out_samples(n, orig, new)
    buf = torch.full((rows * n + GUARD,), float("nan"))
    L.mst_resample_backward(g, rows, n, orig, new, tables(L, orig, new), buf, None)
    assert torch.isnan(buf[rows * n:]).all(), "written past grad_x"
    gx = buf[: rows * n].view(rows, n)
    assert torch.isfinite(gx).all(), "grad_x not fully written"
    return gx


def strided(x):
    """The same rows as a view ``wide[:, 1:-2]`` of a wider buffer: odd 4-byte alignment, row stride > length."""
    wide = noise((x.shape[0], x.shape[1] + 3), 999)
    wide[:, 1:-2] = x
    v = wide[:, 1:-2]
    assert v.stride(0) == x.shape[1] + 3 and (v.data_ptr() // 4) % 4 != (wide.data_ptr() // 4) % 4
    return v


# ---- 1. + 2. values and lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", RATIOS)
def test_forward_matches_the_float64_restatement(lib, orig, new, record):
    F = int(tables(lib, orig, new)[4])  # frames per tile of the forward (include/diffmst_hip.h)
    assert F % 4 == 0 and F > 0
    worst = 0.0
    for n in case_lengths(orig, new, F):
        x = noise((1, n), 1000 + n)
        worst = max(worst, check_forward(lambda v: forward(lib, v, orig, new), orig, new, x, f"{orig}->{new} 1x{n}"))
    o, _ = R.reduced(orig, new)
    for n in (o + 1, 5003):
        x = noise((3, n), 2000 + n)
        worst = max(worst, check_forward(lambda v: forward(lib, v, orig, new), orig, new, x, f"{orig}->{new} 3x{n}"))
        worst = max(worst, check_forward(lambda v: forward(lib, strided(v), orig, new), orig, new, x, f"{orig}->{new} 3x{n} strided"))
    x = noise((2, 3, 5003), 3000)  # two leading dimensions: six rows of one buffer
    worst = max(worst, check_forward(lambda v: forward(lib, v.view(6, -1), orig, new).view(2, 3, -1), orig, new, x, f"{orig}->{new} 2x3x5003"))
    record(err=worst, bound=R.forward_bound(orig, new))


@pytest.mark.parametrize("orig,new", RATIOS)
def test_tap_counts_of_the_table(lib, orig, new):
    """T of the device table = the restatement's longest run of coefficients that are not exactly zero; the same for the adjoint."""
    t = tables(lib, orig, new)
    o, n = R.reduced(orig, new)
    assert (int(t[0]), int(t[1]), int(t[2])) == (o, n, R.sinc_kernel(orig, new)[1])
    assert int(t[3]) == R.forward_stats(orig, new)[0]
    assert int(t[5]) == R.adjoint_stats(orig, new)[0]
    expect = {(88200, 44100): (25,), (96000, 44100): (27,), (44100, 16000): (34,), (44100, 8000): (67,)}
    assert int(t[3]) in expect.get((orig, new), (13, 14))  # 48000 <-> 44100 and every up-conversion to 44100: 13 or 14


def test_out_samples(lib):
    for orig, new in RATIOS:
        o, n = R.reduced(orig, new)
        for L in (1, 2, o - 1, o, o + 1, 5003, 524288, 10584000, (1 << 31) + 7):
            if L >= 1:
                assert lib.mst_resample_out_samples(L, orig, new) == (n * L + o - 1) // o
    assert lib.mst_resample_out_samples(1000, 44100, 44100) == 1000
    assert lib.mst_resample_out_samples(0, 48000, 44100) == 0


# ---- 3. closed form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", SINE_RATIOS)
def test_sine_matches_the_closed_form(lib, orig, new, record):
    x, want, mid = sine_case(orig, new)
    ref = float((R.resample(x, orig, new, torch.float64) - want)[mid].abs().max())
    got = forward(lib, x.float().view(1, -1), orig, new)[0].double()
    err = float((got - want)[mid].abs().max())
    print(f"\n[997 Hz {orig}->{new}] restatement vs closed form {ref:.3e}, kernel {err:.3e}")
    record(restatement=ref, kernel=err)
    assert ref <= RESTATEMENT_VS_CLOSED_FORM
    assert err <= RESTATEMENT_VS_CLOSED_FORM + R.forward_bound(orig, new)


# ---- 4. adjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", RATIOS)
def test_adjoint(lib, orig, new, record):
    o, _ = R.reduced(orig, new)
    for n in (o + 1, 5003):
        x = noise((3, n), 4000 + n)
        g = noise((3, R.out_samples(n, orig, new)), 5000 + n)
        want = R.adjoint(g, n, orig, new)
        gx = backward(lib, g, n, orig, new)
        bound_adj = R.adjoint_bound(orig, new, float(g.abs().max()))
        err = float((gx.double() - want).abs().max())
        print(f"\n[{orig}->{new} adjoint 3x{n}] |gx - gx_f64| = {err:.3e} (bound {bound_adj:.3e})")
        assert err <= bound_adj
        # <A x, g> = <x, A^T g>, both sides from the fp32 results, summed in float64
        y = forward(lib, x, orig, new)
        lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
        slack = R.forward_bound(orig, new, float(x.abs().max())) * float(g.abs().sum()) + bound_adj * float(x.abs().sum())
        print(f"[{orig}->{new} dot 3x{n}] <Ax, g> - <x, A^T g> = {lhs - rhs:.3e} (bound {slack:.3e})")
        assert abs(lhs - rhs) <= slack
    record(err=err, bound=R.adjoint_bound(orig, new))


# ---- 5. determinism and batching ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(48000, 44100), (44100, 48000), (44100, 8000)])
def test_bit_identical_calls_and_rows(lib, orig, new):
    x = noise((3, 5003), 6000)
    a, b = forward(lib, x, orig, new), forward(lib, x, orig, new)
    assert torch.equal(a, b)
    g = noise(tuple(a.shape), 6001)
    ga, gb = backward(lib, g, 5003, orig, new), backward(lib, g, 5003, orig, new)
    assert torch.equal(ga, gb)
    for r in range(3):
        assert torch.equal(forward(lib, x[r:r + 1], orig, new)[0], a[r])
        assert torch.equal(backward(lib, g[r:r + 1].contiguous(), 5003, orig, new)[0], ga[r])


# ---- 6. edges -----------------------------------------------------------------------------------------------------------------
def test_unsupported_ratio_launches_nothing(lib):
    from mst import _cabi

    assert lib.mst_resample_tables_bytes(44101, 44100) == 0 and lib.mst_resample_out_samples(1000, 44101, 44100) == 0
    assert lib.mst_resample_tables_bytes(44100, 44100) == 0  # equal rates: nothing to launch
    assert lib.mst_resample_tables_bytes(1024, 1) == 0       # 12413 taps per output
    assert lib.mst_resample_tables_bytes(1024, 1023) > 0 and lib.mst_resample_tables_bytes(3, 1024) > 0  # the corners of the domain
    x, y, t = torch.ones(1, 1000), torch.full((1100,), float("nan")), torch.zeros(64, dtype=torch.int32)
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_resample_init_tables(44101, 44100, t, None)
    assert e.value.code != 0
    assert not t.any()
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_resample_forward(x, 1, 1000, 1000, 44101, 44100, t, y, None)
    assert e.value.code != 0
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_resample_backward(x, 1, 1000, 44101, 44100, t, y, None)
    assert e.value.code != 0
    assert torch.isnan(y).all()
    with pytest.raises(_cabi.AbiError) as e:
        lib.mst_resample_forward(None, 1, 1000, 1000, 48000, 44100, None, None, None)
    assert e.value.code != 0


@pytest.mark.parametrize("orig,new", [(1024, 1023), (3, 1024), (1000, 97)])
def test_corners_of_the_domain(lib, orig, new):
    """The largest reduced rates, a long adjoint run (3 -> 1024: 4000+ entries per input sample, no LDS) and ~124 taps."""
    x = noise((2, 2 * orig + 5), 7000)
    check_forward(lambda v: forward(lib, v, orig, new), orig, new, x, f"{orig}->{new}")
    g = noise((2, R.out_samples(x.shape[1], orig, new)), 7001)
    err = float((backward(lib, g, x.shape[1], orig, new).double() - R.adjoint(g, x.shape[1], orig, new)).abs().max())
    assert err <= R.adjoint_bound(orig, new, float(g.abs().max()))


def test_wrapper_argument_checks():
    import mst.utils as U

    x = torch.zeros(2, 100)
    assert U.resample(x, 44100, 44100) is x and U.resample(x, 44100.0, 44100) is x and U.Resample(48000, 48000)(x) is x
    for bad in (44100.5, "44100", None, 0, -48000, float("nan"), True):
        with pytest.raises(ValueError):
            U.resample(x, bad, 44100)
        with pytest.raises(ValueError):
            U.resample(x, 48000, bad)
    with pytest.raises(ValueError):
        U.Resample(48000.25, 44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        U.resample(x, 48000, 44100)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        U.Resample(48000, 44100)(x)
    with pytest.raises(TypeError):
        U.resample(torch.zeros(2, 100, dtype=torch.int32), 48000, 44100)
