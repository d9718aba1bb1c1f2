// mst_resample.hip - sample-rate conversion with the semantics of torchaudio.functional.resample at its defaults
// (resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99), forward and adjoint.
// PARITY UNPINNED: restated from torchaudio's published source, never run against the package.
//
// With o = orig / gcd and n = new / gcd the operation is  y[j n + i] = sum_k h[i][k] xpad[j o + k],  i < n, k < K = 2 width + o:
// n phases of a K-tap filter, one frame of n outputs per o inputs.  torchaudio runs it as a dense strided conv1d over all K taps;
// all but a contiguous run of T of them (13..14 for 48000 <-> 44100) are EXACTLY 0.0f once the float64 coefficients are rounded
// to fp32 (|t| clamped to 6 gives ~1e-49), so the kernels below touch only that run.  The adjoint has the same shape with the
// roles swapped: input sample m = q o + r - width gathers E consecutive grad_y samples around q n, one coefficient run per residue r.
// Both directions are therefore ONE tile routine,
//     out[Q p_out + c + shift] = sum_{e < taps} C[e][c] in[Q p_in + first[c] + e],     c < p_out,
// over two tables of the same layout (first[p_out] int32, then C[taps][p_out] fp32, tap-major: consecutive lanes hold consecutive
// c and read consecutive LDS words).  The adjoint table is built from the forward table's fp32 numbers, so A^T uses bit-for-bit
// what A uses.  A workgroup owns one tile of F frames Q (F % 4 == 0): it copies its table and the input span it needs into LDS
// (16-byte loads from the aligned address below the span's start, whatever the row's alignment; samples outside the row are zeros), then
// every lane takes items (c, four frames): one coefficient read and four input reads per tap, `taps` fmaf in ascending tap order
// per output.  Every output is written once; no atomics; a row's result does not depend on the other rows of the call.
// Ratios whose table or span does not fit the LDS pools run the same loop on global memory (slow, correct).
// The coefficient expression is evaluated on the host in float64 exactly as torchaudio writes it and rounded once to fp32: this
// unit is compiled with -ffp-contract=off (Makefile).
#include <math.h>
#include <string.h>

#include <vector>

#include "mst_common.h"

namespace mst {

constexpr int kResWG = 256;
constexpr int kResMaxRate = 1024;   // reduced o and n
constexpr int kResMaxTaps = 132;    // analytic forward run length floor(12 o / base) + 1 (the exact T is never larger)
constexpr int kResHdr = 16;         // int32 words in front of the two tables (include/diffmst_hip.h)
constexpr int kResPools[3] = {6144, 12288, 15872};  // LDS words of the three kernel variants (24 / 48 / 62 KB)

// what a launch needs besides the pointers; a pure function of (o, n) and the direction
struct ResGeo {
    int32_t p_out, p_in;   // outputs / inputs per frame
    int32_t lo, extent;    // first[c] + e lies in [lo, lo + extent) for every c, e
    int32_t shift;         // out index = Q p_out + c + shift
    int32_t F;             // frames per tile
    int32_t tab_word;      // where this direction's table starts in the buffer (int32 words)
    int32_t taps_word;     // header word that holds the exact tap count
    int32_t pool;          // index into kResPools, -1: no LDS
    int64_t q_start;       // first frame of the launch
};

template <int kPool>
__device__ __forceinline__ void res_tile(const float* __restrict__ in, int64_t in_len, float* __restrict__ out, int64_t out_len,
                                         const int32_t* __restrict__ tables, const ResGeo& g, float* __restrict__ pool) {
    const int tid = threadIdx.x, p_out = g.p_out, p_in = g.p_in;
    const int taps = tables[g.taps_word];
    const int32_t* __restrict__ tab = tables + g.tab_word;
    const int64_t Q0 = g.q_start + (int64_t)blockIdx.x * g.F;
    const int64_t s0 = Q0 * p_in + g.lo;  // first input sample any item of the tile may read
    int xoff = -g.lo;                      // LDS word of input sample (Q0 p_in + off) = off + xoff
    const float* xs = nullptr;
    if (kPool > 0) {
        const int tabw = p_out * (taps + 1);
        for (int w = tid; w < tabw; w += kResWG) pool[w] = __int_as_float(tab[w]);
        float* stage = pool + ((tabw + 3) & ~3);
        // 16-byte loads from the aligned address at or below in + s0 (rows start at any 4-byte alignment)
        const int mis = (int)((((uintptr_t)in + (uintptr_t)(s0 * 4)) >> 2) & 3);
        const int64_t a0 = s0 - mis;
        const int span = (g.F - 1) * p_in + g.extent;
        const int nvec = (span + mis + 3) >> 2;
        for (int v = tid; v < nvec; v += kResWG) {
            const int64_t i = a0 + 4 * (int64_t)v;
            float4 q;
            if (i >= 0 && i + 3 < in_len) q = *reinterpret_cast<const float4*>(in + i);
            else {
                q.x = i >= 0 && i < in_len ? in[i] : 0.f;
                q.y = i + 1 >= 0 && i + 1 < in_len ? in[i + 1] : 0.f;
                q.z = i + 2 >= 0 && i + 2 < in_len ? in[i + 2] : 0.f;
                q.w = i + 3 >= 0 && i + 3 < in_len ? in[i + 3] : 0.f;
            }
            *reinterpret_cast<float4*>(stage + 4 * v) = q;
        }
        xs = stage;
        xoff += mis;
        __syncthreads();
    }
    // items (c, group of four frames), dealt to the lanes in order: item w = c + p_out * group
    const int groups = g.F >> 2, dc = kResWG % p_out, dg = kResWG / p_out;
    int c = tid % p_out, gq = tid / p_out;
    while (gq < groups) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (kPool > 0) {
            const int first = __float_as_int(pool[c]);
            const float* cf = pool + p_out + c;
            const float* x0 = xs + (gq * 4) * p_in + first + xoff;
            const float *x1 = x0 + p_in, *x2 = x1 + p_in, *x3 = x2 + p_in;
#pragma unroll 2
            for (int e = 0; e < taps; ++e) {
                const float h = cf[e * p_out];
                a0 = fmaf(h, x0[e], a0);
                a1 = fmaf(h, x1[e], a1);
                a2 = fmaf(h, x2[e], a2);
                a3 = fmaf(h, x3[e], a3);
            }
        } else {
            const int64_t i0 = (Q0 + gq * 4) * p_in + tab[c];
            const int32_t* cf = tab + p_out + c;
            for (int e = 0; e < taps; ++e) {
                const float h = __int_as_float(cf[(int64_t)e * p_out]);
                const int64_t i = i0 + e, i1 = i + p_in, i2 = i1 + p_in, i3 = i2 + p_in;
                a0 = fmaf(h, i >= 0 && i < in_len ? in[i] : 0.f, a0);
                a1 = fmaf(h, i1 >= 0 && i1 < in_len ? in[i1] : 0.f, a1);
                a2 = fmaf(h, i2 >= 0 && i2 < in_len ? in[i2] : 0.f, a2);
                a3 = fmaf(h, i3 >= 0 && i3 < in_len ? in[i3] : 0.f, a3);
            }
        }
        const int64_t o0 = (Q0 + gq * 4) * p_out + c + g.shift, o1 = o0 + p_out, o2 = o1 + p_out, o3 = o2 + p_out;
        if (o0 >= 0 && o0 < out_len) out[o0] = a0;
        if (o1 >= 0 && o1 < out_len) out[o1] = a1;
        if (o2 >= 0 && o2 < out_len) out[o2] = a2;
        if (o3 >= 0 && o3 < out_len) out[o3] = a3;
        c += dc;
        gq += dg;
        if (c >= p_out) {
            c -= p_out;
            ++gq;
        }
    }
}

// grid (tiles, rows).  x rows `row_stride` apart, y dense (rows, n_out)
template <int kPool>
__global__ __launch_bounds__(kResWG) void k_resample_fwd(const float* __restrict__ x, int64_t n_in, int64_t row_stride,
                                                         float* __restrict__ y, int64_t n_out,
                                                         const int32_t* __restrict__ tables, ResGeo g) {
    __shared__ float4 pool[kPool > 0 ? kPool / 4 : 1];
    res_tile<kPool>(x + (int64_t)blockIdx.y * row_stride, n_in, y + (int64_t)blockIdx.y * n_out, n_out, tables, g,
                    reinterpret_cast<float*>(pool));
}
// the adjoint: grad_y dense (rows, n_out) -> grad_x dense (rows, n_in); grad_y beyond n_out counts as zero
template <int kPool>
__global__ __launch_bounds__(kResWG) void k_resample_bwd(const float* __restrict__ grad_y, int64_t n_out, float* __restrict__ grad_x,
                                                         int64_t n_in, const int32_t* __restrict__ tables, ResGeo g) {
    __shared__ float4 pool[kPool > 0 ? kPool / 4 : 1];
    res_tile<kPool>(grad_y + (int64_t)blockIdx.y * n_out, n_out, grad_x + (int64_t)blockIdx.y * n_in, n_in, tables, g,
                    reinterpret_cast<float*>(pool));
}

// the table travels to the device as kernel arguments (no host buffer has to outlive the call, nothing is cached in the library)
constexpr int kResFillWords = 256;
struct ResPiece {
    uint32_t w[kResFillWords];
};
__global__ __launch_bounds__(kResFillWords) void k_resample_fill(uint32_t* __restrict__ dst, int count, ResPiece piece) {
    const int i = threadIdx.x;
    if (i < count) dst[i] = piece.w[i];
}

// ---- host side --------------------------------------------------------------------------------------------------------------
namespace {
struct ResPlan {
    bool ok;
    int o, n, width, K, D;
    int taps_ub, ent_ub;   // upper bounds of the two run lengths, from (o, n) alone: they size the buffer and the LDS plan
    ResGeo fwd, bwd;
    size_t words;          // int32 words of the table buffer
};

int res_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// frames per tile and LDS pool of one direction: the smallest pool that keeps at least 80 % of the lanes busy, else the best
void res_pick_tile(ResGeo& g, int taps_ub) {
    const int tab_ub = (g.p_out * (taps_ub + 1) + 3) & ~3;
    const int f_cap = 4 * ((2048 + g.p_out - 1) / g.p_out);
    g.pool = -1;
    g.F = 4 * ((kResWG + g.p_out - 1) / g.p_out);  // no LDS: one round of items
    double best = 0.0;
    for (int p = 0; p < 3; ++p) {
        double eff_p = 0.0;
        int f_p = 0;
        for (int F = 4; F <= f_cap; F += 4) {
            if ((int64_t)tab_ub + (int64_t)(F - 1) * g.p_in + g.extent + 8 > kResPools[p]) break;
            const int items = g.p_out * (F / 4), rounds = (items + kResWG - 1) / kResWG;
            const double eff = (double)items / ((double)rounds * kResWG);
            if (eff >= eff_p) {
                eff_p = eff;
                f_p = F;
            }
        }
        if (f_p && eff_p > best) {
            best = eff_p;
            g.pool = p;
            g.F = f_p;
        }
        if (best >= 0.8) break;
    }
}

ResPlan res_plan(int32_t orig_freq, int32_t new_freq) {
    ResPlan p{};
    if (orig_freq <= 0 || new_freq <= 0) return p;
    const int g = res_gcd(orig_freq, new_freq);
    p.o = orig_freq / g;
    p.n = new_freq / g;
    if (p.o == p.n || p.o > kResMaxRate || p.n > kResMaxRate) return p;  // equal rates: the identity, the caller's business
    const double base = (double)(p.o < p.n ? p.o : p.n) * 0.99;
    const double taps_an = floor(12.0 * (double)p.o / base) + 1.0;
    if (taps_an > (double)kResMaxTaps) return p;
    p.width = (int)ceil(6.0 * (double)p.o / base);
    p.K = 2 * p.width + p.o;
    p.D = (p.K - 1) / p.o;
    p.taps_ub = (int)taps_an + 2 < p.K ? (int)taps_an + 2 : p.K;
    const int64_t ent = (int64_t)floor(12.0 * (double)p.n / base) + 3, ent_max = (int64_t)(p.D + 1) * p.n;
    p.ent_ub = (int)(ent < ent_max ? ent : ent_max);
    const int fwd_words = (p.n * (p.taps_ub + 1) + 3) & ~3, bwd_words = (p.o * (p.ent_ub + 1) + 3) & ~3;
    p.fwd = ResGeo{p.n, p.o, -p.width, p.K, 0, 0, kResHdr, 3, -1, 0};
    p.bwd = ResGeo{p.o, p.n, -p.D * p.n, (p.D + 1) * p.n, -p.width, 0, kResHdr + fwd_words, 5, -1, p.width / p.o};
    res_pick_tile(p.fwd, p.taps_ub);
    res_pick_tile(p.bwd, p.ent_ub);
    p.words = (size_t)kResHdr + fwd_words + bwd_words;
    p.ok = true;
    return p;
}

// h[i][k] in float64 exactly as torchaudio's _get_sinc_resample_kernel writes it, rounded once to fp32
float res_coefficient(int i, int k, const ResPlan& p) {
    const double base = (double)(p.o < p.n ? p.o : p.n) * 0.99;
    double t = ((double)(k - p.width) / (double)p.o - (double)i / (double)p.n) * base;
    t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
    const double c = cos(t * M_PI / 6.0 / 2.0);
    const double win = c * c;
    t = t * M_PI;
    const double s = t == 0.0 ? 1.0 : sin(t) / t;
    return (float)(s * win * (base / (double)p.o));
}

// both tables.  false when a run is longer than its analytic bound (never seen; the buffer would be too small)
bool res_host_tables(const ResPlan& p, std::vector<int32_t>& buf) {
    const int o = p.o, n = p.n, K = p.K;
    std::vector<float> h((size_t)n * K);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) h[(size_t)i * K + k] = res_coefficient(i, k, p);
    auto bits = [](float f) {
        int32_t v;
        memcpy(&v, &f, 4);
        return v;
    };
    // forward: per phase the run [lo_i, hi_i] of taps that are not exactly zero
    std::vector<int> lo(n, K), hi(n, -1);
    int T = 1;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < K; ++k)
            if (h[(size_t)i * K + k] != 0.0f) {
                lo[i] = lo[i] < k ? lo[i] : k;
                hi[i] = k;
            }
        if (hi[i] >= 0 && hi[i] - lo[i] + 1 > T) T = hi[i] - lo[i] + 1;
    }
    // adjoint: input residue r = (m + width) mod o is reached through k = r + d o from phase i; v = i - d n is the offset of that
    // output from frame q = (m + width) / o.  Run [vlo_r, vhi_r] of offsets whose coefficient is not exactly zero
    const int vmin = -p.D * n;
    std::vector<int> vlo(o, n), vhi(o, vmin - 1);
    int E = 1;
    for (int r = 0; r < o; ++r) {
        for (int d = 0; d <= p.D && r + d * o < K; ++d)
            for (int i = 0; i < n; ++i)
                if (h[(size_t)i * K + r + d * o] != 0.0f) {
                    const int v = i - d * n;
                    vlo[r] = vlo[r] < v ? vlo[r] : v;
                    vhi[r] = vhi[r] > v ? vhi[r] : v;
                }
        if (vhi[r] >= vlo[r] && vhi[r] - vlo[r] + 1 > E) E = vhi[r] - vlo[r] + 1;
    }
    if (T > p.taps_ub || E > p.ent_ub) return false;
    buf.assign(p.words, 0);
    buf[0] = o; buf[1] = n; buf[2] = p.width; buf[3] = T; buf[4] = p.fwd.F; buf[5] = E; buf[6] = p.bwd.F;
    buf[7] = p.fwd.tab_word; buf[8] = p.bwd.tab_word;
    int32_t* f = buf.data() + p.fwd.tab_word;
    for (int i = 0; i < n; ++i) {
        int k0 = hi[i] < 0 ? 0 : lo[i];
        k0 = k0 + T > K ? K - T : k0;  // the padded run stays inside the staged span
        f[i] = k0 - p.width;
        for (int e = 0; e < T; ++e) f[n + (size_t)e * n + i] = bits(h[(size_t)i * K + k0 + e]);
    }
    int32_t* b = buf.data() + p.bwd.tab_word;
    for (int r = 0; r < o; ++r) {
        int v0 = vhi[r] < vlo[r] ? vmin : vlo[r];
        v0 = v0 + E > n ? n - E : v0;
        b[r] = v0;
        for (int e = 0; e < E; ++e) {
            const int v = v0 + e, i = ((v % n) + n) % n, d = (i - v) / n, k = r + d * o;
            b[o + (size_t)e * o + r] = (d >= 0 && d <= p.D && k < K) ? bits(h[(size_t)i * K + k]) : 0;
        }
    }
    return true;
}

int64_t res_out_samples(int64_t L, const ResPlan& p) { return ((int64_t)p.n * L + p.o - 1) / p.o; }

constexpr int64_t kResMaxSamples = (int64_t)1 << 40;
constexpr int kResRowsPerLaunch = 65535;

template <typename Launch>
int res_for_row_chunks(int32_t rows, Launch launch) {
    for (int32_t r0 = 0; r0 < rows; r0 += kResRowsPerLaunch) launch(r0, rows - r0 < kResRowsPerLaunch ? rows - r0 : kResRowsPerLaunch);
    return (int)hipGetLastError();
}
}  // namespace
}  // namespace mst

using namespace mst;

extern "C" size_t mst_resample_tables_bytes(int32_t orig_freq, int32_t new_freq) {
    const ResPlan p = res_plan(orig_freq, new_freq);
    return p.ok ? p.words * 4 : 0;
}
extern "C" int mst_resample_init_tables(int32_t orig_freq, int32_t new_freq, void* tables, void* stream) {
    const ResPlan p = res_plan(orig_freq, new_freq);
    if (!p.ok || !tables) return hipErrorInvalidValue;
    std::vector<int32_t> buf;
    if (!res_host_tables(p, buf)) return hipErrorInvalidValue;
    const int64_t words = (int64_t)buf.size();
    for (int64_t at = 0; at < words; at += kResFillWords) {
        ResPiece piece;
        const int count = (int)(words - at < kResFillWords ? words - at : kResFillWords);
        memset(&piece, 0, sizeof(piece));
        memcpy(piece.w, buf.data() + at, (size_t)count * 4);
        hipLaunchKernelGGL(k_resample_fill, dim3(1), dim3(kResFillWords), 0, (hipStream_t)stream, (uint32_t*)tables + at, count, piece);
    }
    return (int)hipGetLastError();
}
extern "C" int64_t mst_resample_out_samples(int64_t n_samples, int32_t orig_freq, int32_t new_freq) {
    if (n_samples <= 0 || n_samples > kResMaxSamples || orig_freq <= 0 || new_freq <= 0) return 0;
    if (orig_freq == new_freq) return n_samples;
    const ResPlan p = res_plan(orig_freq, new_freq);
    return p.ok ? res_out_samples(n_samples, p) : 0;
}
extern "C" int mst_resample_forward(const float* x, int32_t rows, int64_t n_samples, int64_t row_stride, int32_t orig_freq,
                                    int32_t new_freq, const void* tables, float* y, void* stream_) {
    const ResPlan p = res_plan(orig_freq, new_freq);
    if (!p.ok || !x || !tables || !y || rows <= 0 || n_samples <= 0 || n_samples > kResMaxSamples || row_stride < 0 ||
        ((uintptr_t)x & 3) || ((uintptr_t)tables & 3))
        return hipErrorInvalidValue;
    const int64_t n_out = res_out_samples(n_samples, p);
    const int64_t frames = (n_out + p.n - 1) / p.n, tiles = (frames + p.fwd.F - 1) / p.fwd.F;
    if (tiles > 2147483647) return hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int32_t* tab = (const int32_t*)tables;
    const ResGeo g = p.fwd;
    return res_for_row_chunks(rows, [&](int32_t r0, int32_t nr) {
        const float* xr = x + (int64_t)r0 * row_stride;
        float* yr = y + (int64_t)r0 * n_out;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        switch (g.pool) {
            case 0: hipLaunchKernelGGL(k_resample_fwd<kResPools[0]>, grid, dim3(kResWG), 0, stream, xr, n_samples, row_stride, yr, n_out, tab, g); break;
            case 1: hipLaunchKernelGGL(k_resample_fwd<kResPools[1]>, grid, dim3(kResWG), 0, stream, xr, n_samples, row_stride, yr, n_out, tab, g); break;
            case 2: hipLaunchKernelGGL(k_resample_fwd<kResPools[2]>, grid, dim3(kResWG), 0, stream, xr, n_samples, row_stride, yr, n_out, tab, g); break;
            default: hipLaunchKernelGGL(k_resample_fwd<0>, grid, dim3(kResWG), 0, stream, xr, n_samples, row_stride, yr, n_out, tab, g); break;
        }
    });
}
extern "C" int mst_resample_backward(const float* grad_y, int32_t rows, int64_t n_samples, int32_t orig_freq, int32_t new_freq,
                                     const void* tables, float* grad_x, void* stream_) {
    const ResPlan p = res_plan(orig_freq, new_freq);
    if (!p.ok || !grad_y || !tables || !grad_x || rows <= 0 || n_samples <= 0 || n_samples > kResMaxSamples ||
        ((uintptr_t)grad_y & 3) || ((uintptr_t)tables & 3))
        return hipErrorInvalidValue;
    const int64_t n_out = res_out_samples(n_samples, p);
    const int64_t q_end = (p.width + n_samples - 1) / p.o, frames = q_end - p.bwd.q_start + 1, tiles = (frames + p.bwd.F - 1) / p.bwd.F;
    if (tiles > 2147483647) return hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int32_t* tab = (const int32_t*)tables;
    const ResGeo g = p.bwd;
    return res_for_row_chunks(rows, [&](int32_t r0, int32_t nr) {
        const float* gr = grad_y + (int64_t)r0 * n_out;
        float* xr = grad_x + (int64_t)r0 * n_samples;
        const dim3 grid((unsigned)tiles, (unsigned)nr);
        switch (g.pool) {
            case 0: hipLaunchKernelGGL(k_resample_bwd<kResPools[0]>, grid, dim3(kResWG), 0, stream, gr, n_out, xr, n_samples, tab, g); break;
            case 1: hipLaunchKernelGGL(k_resample_bwd<kResPools[1]>, grid, dim3(kResWG), 0, stream, gr, n_out, xr, n_samples, tab, g); break;
            case 2: hipLaunchKernelGGL(k_resample_bwd<kResPools[2]>, grid, dim3(kResWG), 0, stream, gr, n_out, xr, n_samples, tab, g); break;
            default: hipLaunchKernelGGL(k_resample_bwd<0>, grid, dim3(kResWG), 0, stream, gr, n_out, xr, n_samples, tab, g); break;
        }
    });
}
