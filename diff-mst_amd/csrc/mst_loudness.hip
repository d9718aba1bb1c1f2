// mst_loudness.hip - integrated loudness (ITU-R BS.1770-4 as pyloudnorm.Meter computes it with its defaults: K-weighting,
// 0.4 s gating blocks, 75 % overlap) of `rows` signals of 1..5 channels, and the loudness normalisation built on it.
// PARITY UNPINNED: restated from pyloudnorm's published source, never run against it.
//
// The K-weighting is a constant two-biquad cascade (4 DF2T states), so the recurrence is made time-parallel exactly like the
// console's EQ: a lane filters a chunk of kLoudChunk samples from zero state, a wave (one tile = 64 chunks) scans the chunk end
// states with the powers of the constant 4x4 chunk transition P, and the tiles of a signal are chained by a small carry scan.
// Four launches, no workgroup waits for another inside a launch:
//   k_loud_zs     per tile: zero-state pass + in-wave scan -> every lane's start state for a ZERO tile start, and the tile aggregate
//   k_loud_carry  per signal: true start state of every tile (one wave, scan over 64 tiles at a time with powers of T = P^64)
//   k_loud_run    per tile: lane start = zero-start state + P^lane (tile start); filter, square, and sum straight into the two
//                 parts of the tile that lie before / after the one gating-block boundary a tile can hold (the filtered signal is
//                 never written); fixed-order wave sums
//   k_loud_gate   per row, one wave: block energies from the tile parts, block loudness, absolute and relative gate, the two
//                 gated means and the log10, all in float64
// mst_loudness_windows adds a fifth for the gated loudness of every window of a song:
//   k_loud_windows per (window, row), one wave: both gates over the window's complete blocks, from the float64 block energies and
//                 block loudness k_loud_gate left in the workspace - the song is filtered once, the filter is warm at a window's start
// mst_loudness_range adds a fifth of its own for short-term loudness and the EBU Tech 3342 loudness range:
//   k_loud_range   per row, one workgroup: the energy of every 3 s window from the tile parts k_loud_run left, both gates, and the two
//                 percentiles picked by rank - float64, fixed order
// The block boundaries are NOT re-derived on the device: the table holds int(T_g * (j * 0.25) * rate) for every j, evaluated on
// the host in float64 exactly as pyloudnorm writes it (block j = [bound[j], bound[j + 4]), clipped to the signal).
// Precision: the recursion, its carries and every sum run in FLOAT64 (input and outputs are fp32).  The 38 Hz high pass has a
// double pole at 1 - 0.0027: rounding noise injected into its state is amplified ~3600 times (sum of the squared impulse response
// of 1 / A(z)), and after a 30 dB level drop the noise left over from the loud stretch rings on for hundreds of samples - an
// fp32 recursion measured 5.9e-5 .. 8.9e-5 LU off on the first quiet gating block, at the tests' bound of 8.7e-5.
// This unit is compiled with -ffp-contract=off (Makefile): every multiply-add of the filter is an explicit fma, and the
// host-side table arithmetic must not be contracted.
#include <math.h>
#include <string.h>

#include <memory>

#include "mst_common.h"

namespace mst {

constexpr int kLoudChunk = 32;                 // samples one lane filters sequentially
constexpr int kLoudTile = 64 * kLoudChunk;     // samples of one single-wave workgroup (2048)
constexpr int kLoudMaxBounds = 4096;           // boundaries in the table: signals of up to 4092 gating blocks (~409 s at 44.1 kHz)
constexpr int kLoudMaxCh = 5;
constexpr int kLoudStride = kLoudChunk + 1;    // LDS row of one chunk (+1: the lanes' sequential reads hit 64 different banks)

// the table buffer (bytes), filled by mst_loudness_init_tables
struct LoudTables {
    int32_t bounds[kLoudMaxBounds];  // bounds[k] = int(0.4 * (k * 0.25) * rate), float64 on the host
    double denom;                    // T_g * rate
    double pad_;
    double coef[10];                 // 2 x {b0 b1 b2 a1 a2}
    double ppow[6][16];              // P^(2^j), P = (one-sample transition)^kLoudChunk, row-major 4x4
    double tpow[6][16];              // T^(2^j), T = P^64
    double plane[64][16];            // P^lane
};

// one DF2T biquad step in float64 (mst_common.h biquad_step with explicit fused multiply-adds)
__device__ __forceinline__ double loud_biquad(double x, const double* c, double& s1, double& s2) {
    const double y = fma(c[0], x, s1);
    s1 = fma(-c[3], y, fma(c[1], x, s2));
    s2 = fma(-c[4], y, c[2] * x);
    return y;
}
// acc += M v, M row-major 4x4 at a wave-uniform or lane-private address
__device__ __forceinline__ void loud_matvec_acc(const double* __restrict__ M, const double* v, double* acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = acc[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) s = fma(M[i * 4 + k], v[k], s);
        acc[i] = s;
    }
}

// index k of the segment [bounds[k], bounds[k + 1]) that holds sample a (bounds ascend by ~rate / 10; the estimate is corrected
// against the table, never trusted); kLoudMaxBounds - 1 past the last boundary
__device__ __forceinline__ int loud_segment(const int32_t* __restrict__ bounds, int64_t a, int rate) {
    int k = (int)(a * 10 / rate);
    k = k > kLoudMaxBounds - 1 ? kLoudMaxBounds - 1 : k;
    while (k + 1 < kLoudMaxBounds && bounds[k + 1] <= a) ++k;
    while (k > 0 && bounds[k] > a) --k;
    return k;
}
// first boundary above sample a (INT64_MAX-like when there is none)
__device__ __forceinline__ int64_t loud_next_bound(const int32_t* __restrict__ bounds, int64_t a, int rate) {
    const int k = loud_segment(bounds, a, rate);
    return k + 1 < kLoudMaxBounds ? (int64_t)bounds[k + 1] : (int64_t)1 << 62;
}

// one tile of one signal, coalesced 16-byte loads -> LDS -> this lane's chunk in registers
__device__ __forceinline__ void loud_load_chunk(const float* __restrict__ sig, int64_t base, int64_t n, float* __restrict__ lds,
                                                int lane, float* xs) {
#pragma unroll
    for (int q = 0; q < kLoudChunk / 4; ++q) {
        const int p = (q * 64 + lane) * 4;  // position inside the tile
        const float4 v = load4(sig, base + p, n);
        float* d = lds + (p / kLoudChunk) * kLoudStride + (p % kLoudChunk);  // four samples of one chunk (kLoudChunk % 4 == 0)
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < kLoudChunk; ++i) xs[i] = lds[lane * kLoudStride + i];
    wave_lds_sync();
}

// inclusive scan over the lanes of a wave of  v[l] = M v[l - 1] + v[l],  pw[j] = M^(2^j)
__device__ __forceinline__ void loud_wave_scan(double* v, const double* __restrict__ pw, int lane) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int off = 1 << j;
        double o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = __shfl_up(v[d], (unsigned)off);
        if (lane >= off) loud_matvec_acc(pw + j * 16, o, v);
    }
}

__device__ __forceinline__ const float* loud_signal(const float* x, int s, int channels, int64_t row_stride, int64_t channel_stride) {
    return x + (int64_t)(s / channels) * row_stride + (int64_t)(s % channels) * channel_stride;
}

// grid (tiles, signals).  excl: [signal][tile][4][64] start state of every lane for a zero tile start; agg: [signal][tile][4]
__global__ __launch_bounds__(64) void k_loud_zs(const float* __restrict__ x, int channels, int64_t n, int64_t row_stride,
                                                int64_t channel_stride, const LoudTables* __restrict__ tab,
                                                double* __restrict__ excl, double* __restrict__ agg) {
    __shared__ float lds[64 * kLoudStride];
    const int lane = threadIdx.x, tile = blockIdx.x, s = blockIdx.y, ntiles = gridDim.x;
    const float* sig = loud_signal(x, s, channels, row_stride, channel_stride);
    float xs[kLoudChunk];
    loud_load_chunk(sig, (int64_t)tile * kLoudTile, n, lds, lane, xs);
    double c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = tab->coef[i];
    double st[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kLoudChunk; ++i) {
        const double y = loud_biquad((double)xs[i], c, st[0], st[1]);
        loud_biquad(y, c + 5, st[2], st[3]);
    }
    loud_wave_scan(st, &tab->ppow[0][0], lane);  // st: state at the END of this lane's chunk, tile started from zero
    const int64_t t = (int64_t)s * ntiles + tile;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const double prev = __shfl_up(st[d], 1u);
        excl[(t * 4 + d) * 64 + lane] = lane ? prev : 0.0;
        if (lane == 63) agg[t * 4 + d] = st[d];
    }
}

// grid (signals).  start[signal][tile][4] = state at the first sample of the tile
__global__ __launch_bounds__(64) void k_loud_carry(const double* __restrict__ agg, double* __restrict__ start, int ntiles,
                                                   const LoudTables* __restrict__ tab) {
    const int lane = threadIdx.x, s = blockIdx.x;
    const double* a = agg + (int64_t)s * ntiles * 4;
    double* o = start + (int64_t)s * ntiles * 4;
    double carry[4] = {0.0, 0.0, 0.0, 0.0};  // start state of tile g (wave-uniform)
    for (int g = 0; g < ntiles; g += 64) {
        const int tile = g + lane;
        double v[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) v[d] = tile < ntiles ? a[tile * 4 + d] : 0.0;
        if (lane == 0) loud_matvec_acc(&tab->tpow[0][0], carry, v);  // the group's start state enters through its first tile
        loud_wave_scan(v, &tab->tpow[0][0], lane);                 // v: state at the END of tile g + lane
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const double prev = __shfl_up(v[d], 1u);
            if (tile < ntiles) o[tile * 4 + d] = lane ? prev : carry[d];
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) carry[d] = __shfl(v[d], 63);
    }
}

// grid (tiles, signals).  part[signal][tile][2] = sum of y^2 over the samples of the tile below / from its boundary on
__global__ __launch_bounds__(64) void k_loud_run(const float* __restrict__ x, int channels, int64_t n, int64_t row_stride,
                                                 int64_t channel_stride, int rate, const LoudTables* __restrict__ tab,
                                                 const double* __restrict__ excl, const double* __restrict__ start,
                                                 double* __restrict__ part) {
    __shared__ float lds[64 * kLoudStride];
    const int lane = threadIdx.x, tile = blockIdx.x, s = blockIdx.y, ntiles = gridDim.x;
    const float* sig = loud_signal(x, s, channels, row_stride, channel_stride);
    const int64_t base = (int64_t)tile * kLoudTile;
    float xs[kLoudChunk];
    loud_load_chunk(sig, base, n, lds, lane, xs);
    const int64_t t = (int64_t)s * ntiles + tile;
    double st[4], ts[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        st[d] = excl[(t * 4 + d) * 64 + lane];
        ts[d] = start[t * 4 + d];
    }
    loud_matvec_acc(&tab->plane[lane][0], ts, st);
    double c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = tab->coef[i];
    // samples [base, lim0) go to part 0, [lim0, lim1) to part 1; a tile is shorter than the distance of two boundaries
    const int64_t bnd = loud_next_bound(tab->bounds, base, rate);
    const int64_t i0 = base + (int64_t)lane * kLoudChunk;
    const int lim1 = (int)(n - i0 < kLoudChunk ? (n - i0 < 0 ? 0 : n - i0) : kLoudChunk);
    const int lim0 = (int)(bnd - i0 < lim1 ? (bnd - i0 < 0 ? 0 : bnd - i0) : lim1);
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
    for (int i = 0; i < kLoudChunk; ++i) {
        const double u = loud_biquad((double)xs[i], c, st[0], st[1]);
        const double y = loud_biquad(u, c + 5, st[2], st[3]);
        acc0 = fma(y, i < lim0 ? y : 0.0, acc0);
        acc1 = fma(y, (i >= lim0 && i < lim1) ? y : 0.0, acc1);
    }
    const double p0 = wave_sum_f64(acc0), p1 = wave_sum_f64(acc1);
    if (lane == 0) {
        part[t * 2] = p0;
        part[t * 2 + 1] = p1;
    }
}

// energy of the samples [lo, hi) of one signal from its tile parts (lo, hi: boundaries of the table, hi already clipped to n)
__device__ __forceinline__ double loud_block_sum(const double* __restrict__ part, const int32_t* __restrict__ bounds, int64_t lo,
                                                 int64_t hi, int rate) {
    double sum = 0.0;
    if (hi <= lo) return sum;
    for (int64_t t = lo / kLoudTile; t <= (hi - 1) / kLoudTile; ++t) {
        const int64_t a = t * kLoudTile, bnd = loud_next_bound(bounds, a, rate);
        if (a >= lo && a < hi) sum += part[t * 2];                              // [a, min(bnd, tile end)): ends at or before hi
        if (bnd < a + kLoudTile && bnd >= lo && bnd < hi) sum += part[t * 2 + 1];  // [bnd, tile end)
    }
    return sum;
}

// grid (rows), one wave.  zb: [row][channel][nblocks] float64 block energies (scratch)
__global__ __launch_bounds__(64) void k_loud_gate(const double* __restrict__ part, int channels, int64_t n, int ntiles, int nblocks,
                                                  int rate, const LoudTables* __restrict__ tab, double* __restrict__ zb,
                                                  float* __restrict__ lufs, float* __restrict__ block_loudness) {
    const int lane = threadIdx.x, row = blockIdx.x;
    const double gch[kLoudMaxCh] = {1.0, 1.0, 1.0, 1.41, 1.41};
    double* z = zb + (int64_t)row * channels * nblocks;
    double* lj = zb + (int64_t)gridDim.x * channels * nblocks + (int64_t)row * nblocks;  // block loudness, float64
    double sum[kLoudMaxCh], cnt = 0.0;
#pragma unroll
    for (int c = 0; c < kLoudMaxCh; ++c) sum[c] = 0.0;
    // block energies, block loudness, absolute gate
    for (int j = lane; j < nblocks; j += 64) {
        const int64_t lo = tab->bounds[j], hi0 = tab->bounds[j + 4], hi = hi0 < n ? hi0 : n;
        double zc[kLoudMaxCh], w = 0.0;
#pragma unroll
        for (int c = 0; c < kLoudMaxCh; ++c) {
            zc[c] = 0.0;
            if (c < channels) {
                zc[c] = loud_block_sum(part + ((int64_t)row * channels + c) * ntiles * 2, tab->bounds, lo, hi, rate) / tab->denom;
                z[(int64_t)c * nblocks + j] = zc[c];
                w += gch[c] * zc[c];
            }
        }
        const double l = -0.691 + 10.0 * log10(w);
        lj[j] = l;
        if (block_loudness) block_loudness[(int64_t)row * nblocks + j] = (float)l;
        if (l >= -70.0) {
            cnt += 1.0;
#pragma unroll
            for (int c = 0; c < kLoudMaxCh; ++c) sum[c] += zc[c];
        }
    }
    cnt = wave_sum_f64(cnt);
    double w = 0.0;
#pragma unroll
    for (int c = 0; c < kLoudMaxCh; ++c) {
        const double tot = wave_sum_f64(sum[c]);
        w += gch[c] * (cnt > 0.0 ? tot / cnt : 0.0);  // mean of an empty set counts as 0 (pyloudnorm: nan_to_num)
        sum[c] = 0.0;
    }
    const double gamma_r = -0.691 + 10.0 * log10(w) - 10.0;
    // relative gate (every lane re-reads what it wrote itself)
    cnt = 0.0;
    for (int j = lane; j < nblocks; j += 64) {
        const double l = lj[j];
        if (l > gamma_r && l > -70.0) {
            cnt += 1.0;
#pragma unroll
            for (int c = 0; c < kLoudMaxCh; ++c)
                if (c < channels) sum[c] += z[(int64_t)c * nblocks + j];
        }
    }
    cnt = wave_sum_f64(cnt);
    w = 0.0;
#pragma unroll
    for (int c = 0; c < kLoudMaxCh; ++c) {
        const double tot = wave_sum_f64(sum[c]);
        w += gch[c] * (cnt > 0.0 ? tot / cnt : 0.0);
    }
    if (lane == 0) lufs[row] = (float)(-0.691 + 10.0 * log10(w));
}

// one gate of one window: loudness of the mean energy of the blocks [first, first + count) that pass it.  The lanes stride over the
// blocks and both sums are fixed-order, exactly as k_loud_gate forms them (a window of all the blocks is its result bit for bit)
template <bool kRelative>
__device__ __forceinline__ double loud_window_gate(const double* __restrict__ z, const double* __restrict__ lj, int channels, int nblocks,
                                                   int first, int count, double gamma_r, int lane) {
    const double gch[kLoudMaxCh] = {1.0, 1.0, 1.0, 1.41, 1.41};
    double sum[kLoudMaxCh], cnt = 0.0;
#pragma unroll
    for (int c = 0; c < kLoudMaxCh; ++c) sum[c] = 0.0;
    for (int i = lane; i < count; i += 64) {
        const int j = first + i;
        const double l = lj[j];
        if (kRelative ? (l > gamma_r && l > -70.0) : (l >= -70.0)) {
            cnt += 1.0;
#pragma unroll
            for (int c = 0; c < kLoudMaxCh; ++c)
                if (c < channels) sum[c] += z[(int64_t)c * nblocks + j];
        }
    }
    cnt = wave_sum_f64(cnt);
    double w = 0.0;
#pragma unroll
    for (int c = 0; c < kLoudMaxCh; ++c) {
        const double tot = wave_sum_f64(sum[c]);
        w += gch[c] * (cnt > 0.0 ? tot / cnt : 0.0);
    }
    return -0.691 + 10.0 * log10(w);
}

// grid (windows, rows), one wave per window.  Reads what k_loud_gate left in zb (block energies and block loudness, float64); window w
// is the blocks [w * hop, w * hop + wblocks), all of them complete (the host counts only those)
__global__ __launch_bounds__(64) void k_loud_windows(const double* __restrict__ zb, int channels, int nblocks, int wblocks, int hop,
                                                     float* __restrict__ window_lufs) {
    const int lane = threadIdx.x, w = blockIdx.x, row = blockIdx.y, rows = gridDim.y, nw = gridDim.x;
    const double* z = zb + (int64_t)row * channels * nblocks;
    const double* lj = zb + (int64_t)rows * channels * nblocks + (int64_t)row * nblocks;
    const int first = w * hop;
    const double gamma_r = loud_window_gate<false>(z, lj, channels, nblocks, first, wblocks, 0.0, lane) - 10.0;
    const double l = loud_window_gate<true>(z, lj, channels, nblocks, first, wblocks, gamma_r, lane);
    if (lane == 0) window_lufs[(int64_t)row * nw + w] = (float)l;
}

constexpr int kRangeWG = 256;
constexpr int kRangeMax = 4096;  // short-term windows of a signal: at most kLoudMaxBounds - 30 of them

// sum over the workgroup in a fixed order (lane order inside a wave, then wave 0, 1, ...), the same value in every lane
__device__ __forceinline__ double range_block_sum(double v, double* scratch) {
    v = wave_sum_f64(v);
    __syncthreads();  // the last round's readers are done with scratch
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = scratch[0];
#pragma unroll
    for (int w = 1; w < kRangeWG / 64; ++w) t += scratch[w];
    return t;
}
__device__ __forceinline__ double loud_of_energy(double e) { return -0.691 + 10.0 * log10(e); }

// grid (rows), after the meter's four launches.  Short-term window k = samples [bound[k hop], bound[k hop + 30]) (3 s); its energy
// comes from the tile parts k_loud_run left, through the span helper k_loud_gate uses.  EBU Tech 3342: absolute gate l >= -70, relative
// gate l >= -20 + loudness of the mean energy of the absolutely gated windows, LRA = l(95th) - l(10th percentile) of the survivors.
// The percentiles are picked by RANK: a survivor's rank is the number of survivors with a smaller energy (or an equal one and a
// smaller index), which is its place in the ascending sort - exact, no ordering of floating-point sums involved, ties cannot change a
// value.  Everything in float64; nothing read here was left by an earlier call.
__global__ __launch_bounds__(kRangeWG) void k_loud_range(const double* __restrict__ part, int channels, int ntiles, int nshort, int hop,
                                                         int rate, const LoudTables* __restrict__ tab, float* __restrict__ short_term,
                                                         float* __restrict__ range_lu, float* __restrict__ range_bounds) {
    __shared__ double e[kRangeMax];  // window energies; -1 once a gate has removed the window
    __shared__ double scratch[kRangeWG / 64];
    __shared__ double picked[2];
    const int tid = threadIdx.x, row = blockIdx.x;
    const double gch[kLoudMaxCh] = {1.0, 1.0, 1.0, 1.41, 1.41};
    const double denom = 30.0 * (double)tab->bounds[1];
    double sum = 0.0, cnt = 0.0;
    for (int k = tid; k < nshort; k += kRangeWG) {
        const int64_t lo = tab->bounds[k * hop], hi = tab->bounds[k * hop + 30];
        double w = 0.0;
        for (int c = 0; c < channels; ++c)
            w += gch[c] * (loud_block_sum(part + ((int64_t)row * channels + c) * ntiles * 2, tab->bounds, lo, hi, rate) / denom);
        const double l = loud_of_energy(w);
        if (short_term) short_term[(int64_t)row * nshort + k] = (float)l;
        const bool in = l >= -70.0;
        e[k] = in ? w : -1.0;
        if (in) {
            sum += w;
            cnt += 1.0;
        }
    }
    sum = range_block_sum(sum, scratch);
    cnt = range_block_sum(cnt, scratch);
    const double gamma_r = loud_of_energy(cnt > 0.0 ? sum / cnt : 0.0) - 20.0;
    double m_ = 0.0;
    for (int k = tid; k < nshort; k += kRangeWG) {  // every lane re-reads what it wrote itself
        if (e[k] >= 0.0 && !(loud_of_energy(e[k]) >= gamma_r)) e[k] = -1.0;
        if (e[k] >= 0.0) m_ += 1.0;
    }
    const int m = (int)range_block_sum(m_, scratch);  // (its barriers publish e)
    if (tid < 2) picked[tid] = 0.0;
    __syncthreads();
    const int want_lo = ((m - 1) * 10 + 50) / 100, want_hi = ((m - 1) * 95 + 50) / 100;
    for (int k = tid; k < nshort; k += kRangeWG) {
        const double mine = e[k];
        if (mine < 0.0) continue;
        int rank = 0;
        for (int j = 0; j < nshort; ++j) {
            const double o = e[j];
            rank += (o >= 0.0 && (o < mine || (o == mine && j < k))) ? 1 : 0;
        }
        if (rank == want_lo) picked[0] = mine;  // ranks are a permutation of 0 .. m - 1: one writer each
        if (rank == want_hi) picked[1] = mine;
    }
    __syncthreads();
    if (tid == 0) {
        const double l_lo = loud_of_energy(picked[0]), l_hi = loud_of_energy(picked[1]);
        range_lu[row] = m > 0 ? (float)(l_hi - l_lo) : 0.0f;
        if (range_bounds) {
            range_bounds[row * 2] = m > 0 ? (float)l_lo : __int_as_float(0x7fc00000);
            range_bounds[row * 2 + 1] = m > 0 ? (float)l_hi : __int_as_float(0x7fc00000);
        }
    }
}

constexpr int kNormSpan = 256 * 16;  // samples per workgroup

__device__ __forceinline__ bool loud_row_kept(float L, float floor_lufs) {
    return L >= floor_lufs && L > -INFINITY && L < INFINITY;  // a silent row (-inf) is dropped whatever the floor
}

// one workgroup's span of one signal: y = g x, or zeros for a row that is not kept
__device__ __forceinline__ void loud_scale_span(const float* __restrict__ x, float* __restrict__ y, int s, int channels, int64_t n,
                                                int64_t row_stride, int64_t channel_stride, bool kept, float g) {
    const int tid = threadIdx.x;
    const float* xr = loud_signal(x, s, channels, row_stride, channel_stride);
    float* yr = y + (int64_t)s * n;
    const int64_t base = (int64_t)blockIdx.x * kNormSpan;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = base + ((int64_t)r * 256 + tid) * 4;
        if (i >= n) break;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kept) {
            v = load4(xr, i, n);
            v.x *= g; v.y *= g; v.z *= g; v.w *= g;
        }
        store4(yr, i, n, v);
    }
}

// grid (spans, rows * channels).  y dense (rows, channels, n)
__global__ __launch_bounds__(256) void k_loud_normalize(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ lufs, int channels, int64_t n,
                                                        int64_t row_stride, int64_t channel_stride, float target, float floor_lufs,
                                                        uint8_t* __restrict__ keep) {
    const int s = blockIdx.y, row = s / channels, tid = threadIdx.x;
    const float L = lufs[row];
    const bool kept = loud_row_kept(L, floor_lufs);
    const float g = kept ? (float)pow(10.0, ((double)target - (double)L) / 20.0) : 0.0f;
    if (keep && blockIdx.x == 0 && tid == 0 && s % channels == 0) keep[row] = kept ? 1 : 0;
    loud_scale_span(x, y, s, channels, n, row_stride, channel_stride, kept, g);
}

// the same with the gain capped so that the true peak stays at or below `ceiling` dBTP: g = min(10^((target - L) / 20),
// 10^(ceiling / 20) / TP), TP the linear true peak of the row (mst_true_peak).  gain_db (rows): what was applied, -inf for a dropped row
__global__ __launch_bounds__(256) void k_loud_normalize_limited(const float* __restrict__ x, float* __restrict__ y,
                                                                const float* __restrict__ lufs, const float* __restrict__ true_peak,
                                                                int channels, int64_t n, int64_t row_stride, int64_t channel_stride,
                                                                float target, float floor_lufs, float ceiling,
                                                                float* __restrict__ gain_db, uint8_t* __restrict__ keep) {
    const int s = blockIdx.y, row = s / channels, tid = threadIdx.x;
    const float L = lufs[row], tp = true_peak[row];
    const bool kept = loud_row_kept(L, floor_lufs);
    const double g_loud = pow(10.0, ((double)target - (double)L) / 20.0), g_peak = pow(10.0, (double)ceiling / 20.0) / (double)tp;
    const bool capped = tp > 0.0f && g_peak < g_loud;
    const float g = kept ? (float)(capped ? g_peak : g_loud) : 0.0f;
    if (blockIdx.x == 0 && tid == 0 && s % channels == 0) {
        if (keep) keep[row] = kept ? 1 : 0;
        const double db = capped ? (double)ceiling - 20.0 * log10((double)tp) : (double)target - (double)L;
        gain_db[row] = kept ? (float)db : -INFINITY;
    }
    loud_scale_span(x, y, s, channels, n, row_stride, channel_stride, kept, g);
}

// the table travels to the device as kernel arguments (no host buffer has to outlive the call, nothing is cached in the library)
constexpr int kFillWords = 256;
struct LoudPiece {
    uint32_t w[kFillWords];
};
__global__ __launch_bounds__(kFillWords) void k_loud_fill(uint32_t* __restrict__ dst, int count, LoudPiece piece) {
    const int i = threadIdx.x;
    if (i < count) dst[i] = piece.w[i];
}

// ---- host side --------------------------------------------------------------------------------------------------------------
namespace {
typedef double Mat4[4][4];
void mat_mul(const Mat4 a, const Mat4 b, Mat4 o) {
    Mat4 t;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i][k] * b[k][j];
            t[i][j] = s;
        }
    memcpy(o, t, sizeof(Mat4));
}
void mat_store(const Mat4 a, double* o) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[i * 4 + j] = a[i][j];
}

bool loud_rate_ok(int rate) {
    // a tile must be shorter than the smallest distance of two boundaries (~rate / 10 - 1): at most one boundary per tile
    return rate > 0 && rate <= 768000 && (int64_t)rate / 10 - 1 > kLoudTile;
}
// pyloudnorm: numBlocks = int(round((T - T_g) / (T_g * step)) + 1), numpy's round (half to even = nearbyint's default mode)
int loud_num_blocks(int64_t n, int rate) {
    const double T_g = 0.4, step = 0.25, T = (double)n / (double)rate;
    if ((double)n < T_g * (double)rate) return 0;  // "Audio must have length greater than the block size."
    const double nb = nearbyint((T - T_g) / (T_g * step)) + 1.0;
    return nb >= 1.0 && nb + 4.0 <= (double)kLoudMaxBounds ? (int)nb : 0;
}

void loud_host_tables(int rate, LoudTables* T) {
    const double T_g = 0.4, step = 0.25, fs = (double)rate;
    for (int k = 0; k < kLoudMaxBounds; ++k) {
        const double pos = T_g * ((double)k * step) * fs;  // exactly pyloudnorm's expression, float64, no contraction
        T->bounds[k] = pos < 2147483647.0 ? (int32_t)pos : 2147483647;
    }
    T->denom = T_g * fs;
    double* co = T->coef;
    {   // high shelf 4 dB, Q = 1/sqrt(2), 1500 Hz (pyloudnorm IIRfilter "high_shelf")
        const double A = pow(10.0, 4.0 / 40.0), w0 = 2.0 * M_PI * (1500.0 / fs), al = sin(w0) / (2.0 * (1.0 / sqrt(2.0))), c = cos(w0);
        const double a0 = (A + 1) - (A - 1) * c + 2 * sqrt(A) * al;
        co[0] = A * ((A + 1) + (A - 1) * c + 2 * sqrt(A) * al) / a0;
        co[1] = -2 * A * ((A - 1) + (A + 1) * c) / a0;
        co[2] = A * ((A + 1) + (A - 1) * c - 2 * sqrt(A) * al) / a0;
        co[3] = 2 * ((A - 1) - (A + 1) * c) / a0;
        co[4] = ((A + 1) - (A - 1) * c - 2 * sqrt(A) * al) / a0;
    }
    {   // high pass Q = 0.5, 38 Hz ("high_pass")
        const double w0 = 2.0 * M_PI * (38.0 / fs), al = sin(w0) / (2.0 * 0.5), c = cos(w0), a0 = 1 + al;
        co[5] = (1 + c) / 2 / a0;
        co[6] = -(1 + c) / a0;
        co[7] = (1 + c) / 2 / a0;
        co[8] = -2 * c / a0;
        co[9] = (1 - al) / a0;
    }
    // one-sample transition of the state (s1a, s2a, s1b, s2b) at zero input
    const double* cf = T->coef;
    Mat4 M;
    for (int k = 0; k < 4; ++k) {
        double st[4] = {0, 0, 0, 0};
        st[k] = 1.0;
        const double ya = st[0];  // x = 0
        const double a1 = st[1] - cf[3] * ya, a2 = -cf[4] * ya;
        const double yb = cf[5] * ya + st[2];
        const double b1 = cf[6] * ya + st[3] - cf[8] * yb, b2 = cf[7] * ya - cf[9] * yb;
        M[0][k] = a1; M[1][k] = a2; M[2][k] = b1; M[3][k] = b2;
    }
    Mat4 P;
    memcpy(P, M, sizeof(Mat4));
    for (int j = 1; j < kLoudChunk; j <<= 1) mat_mul(P, P, P);  // M^kLoudChunk (a power of two)
    Mat4 Q;
    memset(Q, 0, sizeof(Mat4));
    for (int i = 0; i < 4; ++i) Q[i][i] = 1.0;
    for (int l = 0; l < 64; ++l) {
        mat_store(Q, &T->plane[l][0]);
        mat_mul(P, Q, Q);
    }
    memcpy(Q, P, sizeof(Mat4));
    for (int j = 0; j < 6; ++j) {
        mat_store(Q, &T->ppow[j][0]);
        mat_mul(Q, Q, Q);
    }
    for (int j = 0; j < 6; ++j) {  // Q = P^64 here
        mat_store(Q, &T->tpow[j][0]);
        mat_mul(Q, Q, Q);
    }
}

struct LoudPlan {
    bool ok;
    int ntiles, nblocks;
    int64_t S;
    size_t excl, agg, start, part, zb, total;  // byte offsets
};
LoudPlan loud_plan(int32_t rows, int32_t channels, int64_t n, int32_t rate) {
    LoudPlan p{};
    if (rows <= 0 || rows > 65535 / kLoudMaxCh || channels < 1 || channels > kLoudMaxCh || n <= 0 || n > 2147483647 || !loud_rate_ok(rate))
        return p;
    p.nblocks = loud_num_blocks(n, rate);
    if (p.nblocks <= 0) return p;
    p.ntiles = (int)((n + kLoudTile - 1) / kLoudTile);
    p.S = (int64_t)rows * channels;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += (bytes + 255) / 256 * 256;
        return at;
    };
    p.excl = take((size_t)p.S * p.ntiles * 4 * 64 * sizeof(double));
    p.agg = take((size_t)p.S * p.ntiles * 4 * sizeof(double));
    p.start = take((size_t)p.S * p.ntiles * 4 * sizeof(double));
    p.part = take((size_t)p.S * p.ntiles * 2 * sizeof(double));
    p.zb = take(((size_t)p.S + rows) * p.nblocks * sizeof(double));
    p.total = o;
    p.ok = true;
    return p;
}

// distance of two boundaries when the table is equally spaced (bound[k] == k * bound[1] for every k of the table: 44100, 48000,
// 22050, 32000, 96000, 88200, 24000 Hz among others), 0 otherwise.  The windowed meter counts complete blocks and places windows
// with it, so it takes no other rate.
int loud_even_step(int rate) {
    if (!loud_rate_ok(rate)) return 0;
    const double T_g = 0.4, step = 0.25, fs = (double)rate;
    const int64_t d = (int64_t)(T_g * (1.0 * step) * fs);
    for (int k = 0; k < kLoudMaxBounds; ++k)
        if ((int64_t)(T_g * ((double)k * step) * fs) != (int64_t)k * d) return 0;  // loud_host_tables' expression
    return (int)d;
}

struct LoudWindowsPlan {
    bool ok;
    LoudPlan p;
    int complete, windows;  // complete gating blocks (bound[j + 4] <= n), windows of them
    size_t lufs, total;     // byte offset of the whole-signal loudness nobody asked for; workspace bytes
};
LoudWindowsPlan loud_windows_plan(int32_t rows, int32_t channels, int64_t n, int32_t rate, int32_t wblocks, int32_t hop) {
    LoudWindowsPlan q{};
    const int d = loud_even_step(rate);
    if (d <= 0 || wblocks < 1 || hop < 1) return q;
    q.p = loud_plan(rows, channels, n, rate);
    if (!q.p.ok) return q;
    q.complete = (int)(n / d) - 3;  // n >= 4 d (loud_plan); never more than p.nblocks, which rounds where this floors
    if (q.complete < 1 || q.complete > q.p.nblocks || wblocks > q.complete) return q;
    q.windows = (q.complete - wblocks) / hop + 1;
    q.lufs = q.p.total;
    q.total = q.p.total + ((size_t)rows * sizeof(float) + 255) / 256 * 256;
    q.ok = true;
    return q;
}

// short-term windows of 30 segments of step = rate / 10 samples, hop segments apart: the equally spaced table again
struct LoudRangePlan {
    bool ok;
    LoudPlan p;
    int nshort;
    size_t lufs, total;  // as LoudWindowsPlan
};
LoudRangePlan loud_range_plan(int32_t rows, int32_t channels, int64_t n, int32_t rate, int32_t hop) {
    LoudRangePlan q{};
    const int d = loud_even_step(rate);
    if (d <= 0 || hop < 1 || hop > 30) return q;
    q.p = loud_plan(rows, channels, n, rate);
    if (!q.p.ok) return q;
    const int64_t nseg = n / d;  // at most kLoudMaxBounds - 1 (loud_plan: n / d - 3 <= nblocks <= 4092)
    if (nseg < 30 || nseg > kLoudMaxBounds - 1) return q;
    q.nshort = (int)((nseg - 30) / hop + 1);
    if (q.nshort > kRangeMax) return q;
    q.lufs = q.p.total;
    q.total = q.p.total + ((size_t)rows * sizeof(float) + 255) / 256 * 256;
    q.ok = true;
    return q;
}
}  // namespace
}  // namespace mst

using namespace mst;

extern "C" size_t mst_loudness_tables_bytes(int32_t sample_rate) { return loud_rate_ok(sample_rate) ? sizeof(LoudTables) : 0; }
extern "C" int mst_loudness_init_tables(int32_t sample_rate, void* tables, void* stream) {
    if (!loud_rate_ok(sample_rate) || !tables) return hipErrorInvalidValue;
    static_assert(sizeof(LoudTables) % 4 == 0, "table is copied in 32-bit words");
    std::unique_ptr<LoudTables> T(new LoudTables());
    loud_host_tables(sample_rate, T.get());
    const uint32_t* src = reinterpret_cast<const uint32_t*>(T.get());
    const int words = (int)(sizeof(LoudTables) / 4);
    for (int at = 0; at < words; at += kFillWords) {
        LoudPiece piece;
        const int count = words - at < kFillWords ? words - at : kFillWords;
        memset(&piece, 0, sizeof(piece));
        memcpy(piece.w, src + at, (size_t)count * 4);
        hipLaunchKernelGGL(k_loud_fill, dim3(1), dim3(kFillWords), 0, (hipStream_t)stream, (uint32_t*)tables + at, count, piece);
    }
    return (int)hipGetLastError();
}
extern "C" int32_t mst_loudness_num_blocks(int64_t n_samples, int32_t sample_rate) {
    return loud_rate_ok(sample_rate) && n_samples > 0 ? loud_num_blocks(n_samples, sample_rate) : 0;
}
extern "C" size_t mst_loudness_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate) {
    const LoudPlan p = loud_plan(rows, channels, n_samples, sample_rate);
    return p.ok ? p.total : 0;
}
extern "C" int mst_loudness_integrated(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                                       int64_t channel_stride, int32_t sample_rate, const void* tables, float* lufs,
                                       float* block_loudness, void* workspace, size_t workspace_bytes, void* stream_) {
    const LoudPlan p = loud_plan(rows, channels, n_samples, sample_rate);
    if (!p.ok || !x || !tables || !lufs || !workspace || workspace_bytes < p.total) return hipErrorInvalidValue;
    if (row_stride < 0 || channel_stride < 0 || ((uintptr_t)workspace & 15)) return hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const LoudTables* tab = (const LoudTables*)tables;
    double* excl = (double*)(ws + p.excl);
    double* agg = (double*)(ws + p.agg);
    double* start = (double*)(ws + p.start);
    double* part = (double*)(ws + p.part);
    double* zb = (double*)(ws + p.zb);
    const dim3 grid(p.ntiles, (unsigned)p.S);
    hipLaunchKernelGGL(k_loud_zs, grid, dim3(64), 0, stream, x, (int)channels, n_samples, row_stride, channel_stride, tab, excl, agg);
    hipLaunchKernelGGL(k_loud_carry, dim3((unsigned)p.S), dim3(64), 0, stream, (const double*)agg, start, p.ntiles, tab);
    hipLaunchKernelGGL(k_loud_run, grid, dim3(64), 0, stream, x, (int)channels, n_samples, row_stride, channel_stride,
                       (int)sample_rate, tab, (const double*)excl, (const double*)start, part);
    hipLaunchKernelGGL(k_loud_gate, dim3(rows), dim3(64), 0, stream, (const double*)part, (int)channels, n_samples, p.ntiles,
                       p.nblocks, (int)sample_rate, tab, zb, lufs, block_loudness);
    return (int)hipGetLastError();
}
extern "C" int mst_loudness_num_windows(int64_t n_samples, int32_t sample_rate, int32_t window_blocks, int32_t hop_blocks,
                                        int32_t* num_windows) {
    if (!num_windows) return hipErrorInvalidValue;
    const LoudWindowsPlan q = loud_windows_plan(1, 1, n_samples, sample_rate, window_blocks, hop_blocks);
    *num_windows = q.ok ? q.windows : 0;
    return q.ok ? 0 : hipErrorInvalidValue;
}
extern "C" size_t mst_loudness_windows_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate,
                                                       int32_t window_blocks, int32_t hop_blocks) {
    const LoudWindowsPlan q = loud_windows_plan(rows, channels, n_samples, sample_rate, window_blocks, hop_blocks);
    return q.ok ? q.total : 0;
}
extern "C" int mst_loudness_windows(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                                    int64_t channel_stride, int32_t sample_rate, const void* tables, int32_t window_blocks,
                                    int32_t hop_blocks, float* window_lufs, float* lufs, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
    const LoudWindowsPlan q = loud_windows_plan(rows, channels, n_samples, sample_rate, window_blocks, hop_blocks);
    if (!q.ok || !window_lufs || !workspace || workspace_bytes < q.total) return hipErrorInvalidValue;
    // the song is filtered once: the meter's own four launches leave every block's energy and loudness in the workspace
    float* whole = lufs ? lufs : (float*)((char*)workspace + q.lufs);
    const int status = mst_loudness_integrated(x, rows, channels, n_samples, row_stride, channel_stride, sample_rate, tables, whole,
                                               nullptr, workspace, q.p.total, stream_);
    if (status) return status;
    hipLaunchKernelGGL(k_loud_windows, dim3((unsigned)q.windows, (unsigned)rows), dim3(64), 0, (hipStream_t)stream_,
                       (const double*)((char*)workspace + q.p.zb), (int)channels, q.p.nblocks, (int)window_blocks, (int)hop_blocks,
                       window_lufs);
    return (int)hipGetLastError();
}
extern "C" int mst_loudness_num_short_term(int64_t n_samples, int32_t sample_rate, int32_t hop_segments, int32_t* count) {
    if (!count) return hipErrorInvalidValue;
    const LoudRangePlan q = loud_range_plan(1, 1, n_samples, sample_rate, hop_segments);
    *count = q.ok ? q.nshort : 0;
    return q.ok ? 0 : hipErrorInvalidValue;
}
extern "C" size_t mst_loudness_range_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate,
                                                     int32_t hop_segments) {
    const LoudRangePlan q = loud_range_plan(rows, channels, n_samples, sample_rate, hop_segments);
    return q.ok ? q.total : 0;
}
extern "C" int mst_loudness_range(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                                  int64_t channel_stride, int32_t sample_rate, const void* tables, int32_t hop_segments,
                                  float* short_term_lufs, float* range_lu, float* range_bounds, float* lufs, float* block_loudness,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    const LoudRangePlan q = loud_range_plan(rows, channels, n_samples, sample_rate, hop_segments);
    if (!q.ok || !range_lu || !workspace || workspace_bytes < q.total) return hipErrorInvalidValue;
    // one K-weighting pass: the meter's own four launches, which also write lufs and block_loudness exactly as they always do
    float* whole = lufs ? lufs : (float*)((char*)workspace + q.lufs);
    const int status = mst_loudness_integrated(x, rows, channels, n_samples, row_stride, channel_stride, sample_rate, tables, whole,
                                               block_loudness, workspace, q.p.total, stream_);
    if (status) return status;
    hipLaunchKernelGGL(k_loud_range, dim3((unsigned)rows), dim3(kRangeWG), 0, (hipStream_t)stream_,
                       (const double*)((char*)workspace + q.p.part), (int)channels, q.p.ntiles, q.nshort, (int)hop_segments,
                       (int)sample_rate, (const LoudTables*)tables, short_term_lufs, range_lu, range_bounds);
    return (int)hipGetLastError();
}
extern "C" int mst_loudness_normalize_limited(const float* x, float* y, const float* lufs, const float* true_peak, int32_t rows,
                                              int32_t channels, int64_t n_samples, int64_t row_stride, int64_t channel_stride,
                                              float target_lufs, float floor_lufs, float ceiling_dbtp, float* gain_db, uint8_t* keep,
                                              void* stream_) {
    if (!x || !y || !lufs || !true_peak || !gain_db || rows <= 0 || channels < 1 || channels > kLoudMaxCh ||
        (int64_t)rows * channels > 65535 || n_samples <= 0 || row_stride < 0 || channel_stride < 0 || !(target_lufs == target_lufs) ||
        floor_lufs != floor_lufs || !(ceiling_dbtp == ceiling_dbtp))
        return hipErrorInvalidValue;
    const int64_t nblk = (n_samples + kNormSpan - 1) / kNormSpan;
    if (nblk > 2147483647) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_loud_normalize_limited, dim3((unsigned)nblk, (unsigned)(rows * channels)), dim3(256), 0, (hipStream_t)stream_,
                       x, y, lufs, true_peak, (int)channels, n_samples, row_stride, channel_stride, target_lufs, floor_lufs, ceiling_dbtp,
                       gain_db, keep);
    return (int)hipGetLastError();
}
extern "C" int mst_loudness_normalize(const float* x, float* y, const float* lufs, int32_t rows, int32_t channels,
                                      int64_t n_samples, int64_t row_stride, int64_t channel_stride, float target_lufs,
                                      float floor_lufs, uint8_t* keep, void* stream_) {
    if (!x || !y || !lufs || rows <= 0 || channels < 1 || channels > kLoudMaxCh || (int64_t)rows * channels > 65535 || n_samples <= 0 ||
        row_stride < 0 || channel_stride < 0 || !(target_lufs == target_lufs) || floor_lufs != floor_lufs)
        return hipErrorInvalidValue;
    const int64_t nblk = (n_samples + kNormSpan - 1) / kNormSpan;
    if (nblk > 2147483647) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_loud_normalize, dim3((unsigned)nblk, (unsigned)(rows * channels)), dim3(256), 0, (hipStream_t)stream_, x, y,
                       lufs, (int)channels, n_samples, row_stride, channel_stride, target_lufs, floor_lufs, keep);
    return (int)hipGetLastError();
}
