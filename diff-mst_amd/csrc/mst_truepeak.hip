// mst_truepeak.hip - true peak (ITU-R BS.1770-4 Annex 2) of `rows` items of `channels` signals: the largest magnitude of the signal
// interpolated F times (F = 4 below 96 kHz, 2 below 192 kHz) by a 49-tap Hann-windowed sinc, the interpolator libebur128 uses
// (include/diffmst_hip.h has the definition).  PARITY UNPINNED: written from the published formula, never run against a meter.
//
// The interpolated signal is never written.  Output k = F m + p (phase p) is  y = sum_t h[p + F t] x[m - t],  t = 0 .. 48/F - 1; phase 0
// is the identity (h[24] = 1 and exact zeros), so it is the sample itself.  Two launches:
//   k_true_peak       grid (tiles, rows x channels), 256 lanes.  A workgroup stages the kTpTile positions of its tile and the kTpHalo
//                     samples in front of them into LDS (coalesced 16-byte loads, zeros outside [0, n)); a lane owns kTpRun consecutive
//                     positions, holds them and their history in registers and slides the (F - 1) x 48/F taps over them.  The taps are
//                     kernel arguments: wave-uniform scalars.  Positions run to n + 48/F - 2, so the zero-extended tail after the last
//                     sample is produced by the tile that holds it, or by one more tile.
//   k_true_peak_fold  grid (rows), one wave: the tiles' maxima -> (rows, channels) and (rows), and the sample peak (rows) if asked
// The maximum travels as the BITS of a non-negative float, compared as integers: +inf is 0x7f800000 and a NaN is 0x7fc00000 above it, so
// a NaN survives every fold (fmaxf would drop it) and the result needs no atomics and no order.
// Compiled with -ffp-contract=off (Makefile): the taps are explicit fmaf in a fixed order and the host-side coefficient expression is
// evaluated as written.
#include <math.h>
#include <string.h>

#include "mst_common.h"

namespace mst {

constexpr int kTpRun = 8;                      // consecutive positions one lane owns
constexpr int kTpWG = 256;
constexpr int kTpTile = kTpWG * kTpRun;        // positions of one workgroup
static_assert(kTpTile == MST_TRUE_PEAK_TILE, "the header publishes the tile length");
constexpr int kTpHalo = 24;                    // samples staged in front of a tile: >= 48/F - 1 for both factors, whole runs
constexpr int kTpStride = kTpRun + 1;          // LDS row of one run (+1: the lanes' sequential reads hit 64 different banks)
constexpr int kTpLds = (kTpTile + kTpHalo) / kTpRun * kTpStride;
constexpr int kTpNaN = 0x7fc00000;
static_assert(kTpRun % 4 == 0 && kTpHalo % kTpRun == 0, "16-byte loads land inside one run");

// phase-major taps of the phases 1 .. F - 1:  c[(p - 1) * (48 / F) + t] = h[p + F t]
struct TpTaps {
    float c[48];
};

// integer maximum over the 64 lanes of a wave of values >= 0 (mst_common.h wave_sum's DPP walk; a lane without a source reads 0)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_max_i32(int v) {
    const int o = __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true);
    return o > v ? o : v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
    v = dpp_max_i32<0x111, 0xf>(v);  // row_shr:1
    v = dpp_max_i32<0x112, 0xf>(v);  // row_shr:2
    v = dpp_max_i32<0x114, 0xf>(v);  // row_shr:4
    v = dpp_max_i32<0x118, 0xf>(v);  // row_shr:8
    v = dpp_max_i32<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_max_i32<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

// grid (tiles, rows * channels).  partial[signal][tile][2]: bits of max |y| over the tile's positions and of max |x| over its samples
// (phase 0 alone: the sample peak a meter shows beside the true peak), kTpNaN when a y / an x is NaN
template <int F>
__global__ __launch_bounds__(kTpWG) void k_true_peak(const float* __restrict__ x, int channels, int64_t n, int64_t row_stride,
                                                     int64_t channel_stride, TpTaps taps, int32_t* __restrict__ partial) {
    constexpr int T = 48 / F, NX = kTpRun + T - 1;
    __shared__ float lds[kTpLds];
    __shared__ int32_t wmax[2 * (kTpWG / 64)];
    const int tid = threadIdx.x, tile = blockIdx.x, s = blockIdx.y;
    const float* sig = x + (int64_t)(s / channels) * row_stride + (int64_t)(s % channels) * channel_stride;
    const int64_t base = (int64_t)tile * kTpTile - kTpHalo;  // sample held by LDS element 0
    for (int q = tid; q < (kTpTile + kTpHalo) / 4; q += kTpWG) {
        const int i = q * 4;
        const float4 v = load4_shift(sig, base + i, n);  // zeros in front of the signal and behind it
        float* d = lds + (i / kTpRun) * kTpStride + (i % kTpRun);
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    __syncthreads();
    // X[i] = x[m0 - (T - 1) + i], m0 = this lane's first position
    float X[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        constexpr int first = kTpHalo - (T - 1);
        X[i] = lds[(tid + (first + i) / kTpRun) * kTpStride + (first + i) % kTpRun];
    }
    float m = 0.0f, ms = 0.0f;
    bool bad = false, bad_s = false;
#pragma unroll
    for (int r = 0; r < kTpRun; ++r) {
        const float* w = X + r + T - 1;  // w[-t] = x[m - t]
        ms = fmaxf(ms, fabsf(w[0]));     // phase 0; a NaN here is a NaN in every other phase
        bad_s |= w[0] != w[0];
#pragma unroll
        for (int p = 0; p < F - 1; ++p) {
            const float* c = taps.c + p * T;
            float y;
            if (T <= 12) {
                y = c[0] * w[0];
#pragma unroll
                for (int t = 1; t < T; ++t) y = fmaf(c[t], w[-t], y);
            } else {  // two halves of 12: no sum is more than 13 roundings deep
                float a = c[0] * w[0], b = c[T / 2] * w[-(T / 2)];
#pragma unroll
                for (int t = 1; t < T / 2; ++t) {
                    a = fmaf(c[t], w[-t], a);
                    b = fmaf(c[T / 2 + t], w[-(T / 2 + t)], b);
                }
                y = a + b;
            }
            m = fmaxf(m, fabsf(y));
            bad |= y != y;
        }
    }
    int v = wave_max_i32(bad ? kTpNaN : __float_as_int(fmaxf(m, ms)));
    int vs = wave_max_i32(bad_s ? kTpNaN : __float_as_int(ms));
    if ((tid & 63) == 0) {
        wmax[tid >> 6] = v;
        wmax[kTpWG / 64 + (tid >> 6)] = vs;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < kTpWG / 64; ++i) {
            v = wmax[i] > v ? wmax[i] : v;
            vs = wmax[kTpWG / 64 + i] > vs ? wmax[kTpWG / 64 + i] : vs;
        }
        int32_t* out = partial + ((int64_t)s * gridDim.x + tile) * 2;
        out[0] = v;
        out[1] = vs;
    }
}

// grid (rows), one wave
__global__ __launch_bounds__(64) void k_true_peak_fold(const int32_t* __restrict__ partial, int channels, int64_t ntiles,
                                                       float* __restrict__ true_peak, float* __restrict__ channel_peak,
                                                       float* __restrict__ sample_peak) {
    const int lane = threadIdx.x, row = blockIdx.x;
    int top = 0, top_s = 0;
    for (int c = 0; c < channels; ++c) {
        const int32_t* p = partial + ((int64_t)row * channels + c) * ntiles * 2;
        int v = 0, vs = 0;
        for (int64_t t = lane; t < ntiles; t += 64) {
            v = p[2 * t] > v ? p[2 * t] : v;
            vs = p[2 * t + 1] > vs ? p[2 * t + 1] : vs;
        }
        v = wave_max_i32(v);
        vs = wave_max_i32(vs);
        if (channel_peak && lane == 0) channel_peak[(int64_t)row * channels + c] = __int_as_float(v);
        top = v > top ? v : top;
        top_s = vs > top_s ? vs : top_s;
    }
    if (lane == 0) {
        true_peak[row] = __int_as_float(top);
        if (sample_peak) sample_peak[row] = __int_as_float(top_s);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
namespace {
int tp_factor(int32_t rate) { return rate <= 0 ? 0 : rate < 96000 ? 4 : rate < 192000 ? 2 : 0; }

// h[j] = sinc((j - 24) / F) * 0.5 * (1 - cos(2 pi j / 48)) in float64, rounded once.  The sinc is exact where its argument is a whole
// number (1 at 0, 0 elsewhere: sin(pi k) is rounding noise of pi, not a tap), so phase 0 is the identity
void tp_host_taps(int F, float* h) {
    for (int j = 0; j < 49; ++j) {
        const int k = j - 24;
        double s;
        if (k % F == 0) s = k == 0 ? 1.0 : 0.0;
        else {
            const double t = (double)k / (double)F;
            s = sin(M_PI * t) / (M_PI * t);
        }
        const double w = 0.5 * (1.0 - cos(2.0 * M_PI * (double)j / 48.0));
        h[j] = (float)(s * w);
    }
}

struct TpPlan {
    bool ok;
    int64_t ntiles;
    size_t total;
};
TpPlan tp_plan(int32_t rows, int32_t channels, int64_t n, int32_t factor) {
    TpPlan p{};
    if ((factor != 2 && factor != 4) || rows <= 0 || channels <= 0 || (int64_t)rows * channels > 65535 || n < 1) return p;
    const int64_t positions = n + 48 / factor - 1;  // the last one that can be non-zero is n + 48 / F - 2
    p.ntiles = (positions + kTpTile - 1) / kTpTile;
    if (p.ntiles > 2147483647) return p;
    p.total = ((size_t)rows * channels * (size_t)p.ntiles * 2 * sizeof(int32_t) + 255) / 256 * 256;
    p.ok = true;
    return p;
}
}  // namespace
}  // namespace mst

using namespace mst;

extern "C" int mst_true_peak_factor(int32_t sample_rate, int32_t* factor) {
    if (!factor) return hipErrorInvalidValue;
    *factor = tp_factor(sample_rate);
    return *factor ? 0 : hipErrorInvalidValue;
}
extern "C" int mst_true_peak_coefficients(int32_t factor, float* h49) {
    if ((factor != 2 && factor != 4) || !h49) return hipErrorInvalidValue;
    tp_host_taps(factor, h49);
    return 0;
}
extern "C" size_t mst_true_peak_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t factor) {
    const TpPlan p = tp_plan(rows, channels, n_samples, factor);
    return p.ok ? p.total : 0;
}
extern "C" int mst_true_peak_sample(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                                    int64_t channel_stride, int32_t factor, float* true_peak, float* channel_peak, float* sample_peak,
                                    void* workspace, size_t workspace_bytes, void* stream_) {
    const TpPlan p = tp_plan(rows, channels, n_samples, factor);
    if (!p.ok || !x || !true_peak || !workspace || workspace_bytes < p.total || row_stride < 0 || channel_stride < 0 ||
        ((uintptr_t)workspace & 3))
        return hipErrorInvalidValue;
    float h[49];
    tp_host_taps(factor, h);
    TpTaps taps;
    memset(&taps, 0, sizeof(taps));
    const int T = 48 / factor;
    for (int ph = 1; ph < factor; ++ph)
        for (int t = 0; t < T; ++t) taps.c[(ph - 1) * T + t] = h[ph + factor * t];
    hipStream_t stream = (hipStream_t)stream_;
    int32_t* partial = (int32_t*)workspace;
    const dim3 grid((unsigned)p.ntiles, (unsigned)(rows * channels));
    if (factor == 4)
        hipLaunchKernelGGL(k_true_peak<4>, grid, dim3(kTpWG), 0, stream, x, (int)channels, n_samples, row_stride, channel_stride, taps,
                           partial);
    else
        hipLaunchKernelGGL(k_true_peak<2>, grid, dim3(kTpWG), 0, stream, x, (int)channels, n_samples, row_stride, channel_stride, taps,
                           partial);
    hipLaunchKernelGGL(k_true_peak_fold, dim3((unsigned)rows), dim3(64), 0, stream, (const int32_t*)partial, (int)channels, p.ntiles,
                       true_peak, channel_peak, sample_peak);
    return (int)hipGetLastError();
}
extern "C" int mst_true_peak(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                             int64_t channel_stride, int32_t factor, float* true_peak, float* channel_peak, void* workspace,
                             size_t workspace_bytes, void* stream) {
    return mst_true_peak_sample(x, rows, channels, n_samples, row_stride, channel_stride, factor, true_peak, channel_peak, nullptr,
                                workspace, workspace_bytes, stream);
}
