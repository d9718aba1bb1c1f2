// mst_comp.hip - feed-forward compressor, pan and bus-sum kernels (forward and backward).
//
// Replaces dasp-pytorch's `compressor` / `stereo_panner` + `tracks.sum(dim=2)` (reference call
// sites mst/modules.py:246, 263, 272, 300; algorithm SURVEY A.2/A.5):
//   side = sum_ch x ; x_db = 20 log10(max(|side|,1e-8)) ; soft-knee static curve -> g_c ;
//   g_s[n] = (1-a) g_c[n] + a g_s[n-1] ; y[n] = x[n-L] * 10^((g_s[n]+makeup)/20) .
// Every lane owns kCompChunk = 8 consecutive samples (two 16-byte accesses per stream); the
// one-pole smoother is a first-order linear recurrence handled as zs -> k_scan1 -> run, exactly
// like the EQ states.  The track "apply" kernel loops over the tracks of one mix so the stereo
// bus is accumulated in registers and written once (no (bs,2,T,N) intermediate unless asked for).
#include "mst_kernels.h"
#include "mst_compdev.h"
#include "mst_dev.h"

namespace mst {

constexpr int CC = kCompChunk;

MST_CBR_STAMP_TABLE  // developer timeline, mst_dev.h (nothing in a default build)

// the value is materialised HERE: without it LLVM sinks a whole unrolled loop below the next spin-wait (into the block that uses its
// results), which serialises the arithmetic behind the wait and keeps every operand of the loop alive across it
#if defined(__clang__)
__device__ __forceinline__ void pin(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin2(f2& x) { asm volatile("" : "+v"(x)); }
#else  // host-only g++ build of these sources (the repository's CPU test harness): no code motion to guard against
inline void pin(float&) {}
inline void pin2(f2&) {}
#endif
__device__ __forceinline__ void ld8(const float* row, int64_t i, int64_t n, float* v) {
    const float4 a = load4(row, i, n), b = load4(row, i + 4, n);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void ld8s(const float* row, int64_t i, int64_t n, float* v) {
    const float4 a = load4_shift(row, i, n), b = load4_shift(row, i + 4, n);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(float* row, int64_t i, int64_t n, const float* v);
// Unguarded variants for interior lanes of aligned rows (the overwhelmingly common case): no bounds or
// alignment tests, two plain 16-byte accesses.
__device__ __forceinline__ void ld8f(const float* row, int64_t i, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(row + i), b = *reinterpret_cast<const float4*>(row + i + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8f(float* row, int64_t i, const float* v) {
    *reinterpret_cast<float4*>(row + i) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(row + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
// FAST selects them at compile time inside the kernels: LD8(fast, ...) etc.
template <bool FAST> __device__ __forceinline__ void LD8(const float* row, int64_t i, int64_t n, float* v) {
    if (FAST) ld8f(row, i, v); else ld8(row, i, n, v);
}
template <bool FAST> __device__ __forceinline__ void LD8S(const float* row, int64_t i, int64_t n, float* v) {
    if (FAST) ld8f(row, i, v); else ld8s(row, i, n, v);
}
template <bool FAST> __device__ __forceinline__ void ST8(float* row, int64_t i, int64_t n, const float* v) {
    if (FAST) st8f(row, i, v); else st8(row, i, n, v);
}
__device__ __forceinline__ void st8(float* row, int64_t i, int64_t n, const float* v) {
    store4(row, i, n, make_float4(v[0], v[1], v[2], v[3]));
    store4(row, i + 4, n, make_float4(v[4], v[5], v[6], v[7]));
}

// sum of one value per wave over the workgroup's waves (fixed order), through four LDS floats at `slot`; trailing barrier so that the
// slots may be reused at once.  One-wave workgroups (MST_COMP_WG = 64): the identity, no LDS, no barrier.
__device__ __forceinline__ float waves_sum(float v, float* slot, int tid) {
    if (kCompWaves == 1) return v;
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    lds_barrier();
    float s = 0.0f;
    if constexpr (kCompWaves == 4) s = (slot[0] + slot[1]) + (slot[2] + slot[3]);
    else
        for (int w = 0; w < kCompWaves; ++w) s += slot[w];
    lds_barrier();
    return s;
}

// ---- first-order carry machinery -------------------------------------------------------------------
// Per lane chunk the smoother is  s_out = a s_in + z  (a = alpha^8, z = zero-state end value).
// block_enter<REV>() returns the state ENTERING this lane's chunk given the state S entering the
// workgroup's 2048-sample block: wave-level Hillis-Steele with shuffles, wave aggregates through LDS.
// Scan order is lane-ascending (forward recursion) or lane-descending (REV, the adjoint recursion).
template <bool REV>
__device__ __forceinline__ float block_enter(float z, float a, float log2a, float S, float* lds, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int rl = REV ? 63 - lane : lane, rw = REV ? kCompWaves - 1 - wave : wave;
    float v = z, p = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = REV ? __shfl_down(v, d) : __shfl_up(v, d);
        if (rl >= d) v = fmaf(p, o, v);
        p *= p;
    }
    float sw = S;  // state entering this wave
    if (kCompWaves > 1) {
        if (rl == 63) lds[rw] = v;  // zero-entry aggregate of this wave
        lds_barrier();
        for (int w = 0; w < rw; ++w) sw = fmaf(p, sw, lds[w]);  // p == a^64
    }
    float ex = REV ? __shfl_down(v, 1) : __shfl_up(v, 1);
    if (rl == 0) ex = 0.0f;
    if (kCompWaves > 1) lds_barrier();  // lds may be reused by the caller's next call
    return fmaf(__builtin_amdgcn_exp2f((float)rl * log2a), sw, ex);
}
// The same scan with the entering state S left open: the state entering this lane's chunk is Q0 + W S.  Everything here is known
// before S is (for the in-launch exchange: before the other workgroups' aggregates have arrived).
template <bool REV>
__device__ __forceinline__ void block_enter_split(float z, float a, float log2a, float* lds, int tid, float& Q0, float& W) {
    const int lane = tid & 63, wave = tid >> 6;
    const int rl = REV ? 63 - lane : lane, rw = REV ? kCompWaves - 1 - wave : wave;
    float v = z, p = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = REV ? __shfl_down(v, d) : __shfl_up(v, d);
        if (rl >= d) v = fmaf(p, o, v);
        p *= p;
    }
    float sw = 0.0f;  // zero-entry state entering this wave
    if (kCompWaves > 1) {
        if (rl == 63) lds[rw] = v;
        lds_barrier();
        for (int w = 0; w < rw; ++w) sw = fmaf(p, sw, lds[w]);  // p == a^64
    }
    float ex = REV ? __shfl_down(v, 1) : __shfl_up(v, 1);
    if (rl == 0) ex = 0.0f;
    if (kCompWaves > 1) lds_barrier();
    Q0 = fmaf(__builtin_amdgcn_exp2f((float)rl * log2a), sw, ex);
    W = __builtin_amdgcn_exp2f((float)(rl + 64 * rw) * log2a);
}
// state entering block `blk` from the aggregates of the blocks before it (after it when REV):
//   S = sum_j A^(dist-1) agg[j],  A = a^256, computed in a fixed order by the whole workgroup
template <bool REV>
__device__ __forceinline__ float block_carry(const float* __restrict__ agg, int blk, int nblk, float log2a, float* lds, int tid) {
    float acc = 0.0f;
    if (REV) {
        for (int j = blk + 1 + tid; j < nblk; j += kWG) acc += __builtin_amdgcn_exp2f((float)(j - blk - 1) * (float)kWG * log2a) * agg[j];
    } else {
        for (int j = blk - 1 - tid; j >= 0; j -= kWG) acc += __builtin_amdgcn_exp2f((float)(blk - 1 - j) * (float)kWG * log2a) * agg[j];
    }
    acc = wave_sum(acc);
    return waves_sum(acc, lds + 4, tid);
}

// the same from granules that the other workgroups of THIS launch publish (mst_common.h: gran_publish / gran_wait).  The first poll
// is split off (carry_peek) so that a kernel can request it early, do work that does not need the carry, and only then look at it.
template <bool REV>
__device__ __forceinline__ int carry_first(int blk, int tid) { return REV ? blk + 1 + tid : blk - 1 - tid; }
template <bool REV>
__device__ __forceinline__ gran_t carry_peek(const gran_t* __restrict__ agg, int64_t near_off, int blk, int nblk, int tid) {
    const int j = carry_first<REV>(blk, tid);
    return (j >= 0 && j < nblk) ? gran_load(agg + j + near_off) : 0ull;
}
template <bool REV>
__device__ __forceinline__ float block_carry_g(const gran_t* __restrict__ agg, int64_t near_off, gran_t peek, int blk, int nblk, float log2a, float* lds, int tid,
                                               int32_t* status = nullptr) {
    float acc = 0.0f;
    bool first = true;
    if (REV) {
        for (int j = blk + 1 + tid; j < nblk; j += kWG, first = false) {
            const float v = (first && (peek >> 32) == 1) ? __int_as_float((int)(unsigned)peek) : gran_wait(agg + j, near_off, status);
            acc += __builtin_amdgcn_exp2f((float)(j - blk - 1) * (float)kWG * log2a) * v;
        }
    } else {
        for (int j = blk - 1 - tid; j >= 0; j -= kWG, first = false) {
            const float v = (first && (peek >> 32) == 1) ? __int_as_float((int)(unsigned)peek) : gran_wait(agg + j, near_off, status);
            acc += __builtin_amdgcn_exp2f((float)(blk - 1 - j) * (float)kWG * log2a) * v;
        }
    }
    acc = wave_sum(acc);
    return waves_sum(acc, lds + 4, tid);
}

// zero-entry aggregate of the workgroup's block alone (what the zero-state passes publish): a weighted SUM, not a scan -
//   forward: sum_t a^(255 - t) z_t,   REV: sum_t a^t z_t   (t = lane chunk index in the block, a = alpha^8)
// one exp2, six DPP additions and one barrier instead of block_enter's seven ds_bpermute and two barriers.
template <bool REV>
__device__ __forceinline__ float block_aggregate(float z, float log2a, float* lds, int tid) {
    const float w = __builtin_amdgcn_exp2f((float)(REV ? tid : kWG - 1 - tid) * log2a);
    const float v = wave_sum(w * z);
    return waves_sum(v, lds, tid);
}

// ---- forward: tracks.  grid (nblk, bs).  Accumulates the stereo bus over the T tracks of mix b.
// The loop over the tracks is software-pipelined: track t + 1's EQ output (at both offsets) is requested before track t's block scans, so
// its memory round trip hides behind four barriers and the static-curve arithmetic instead of opening every iteration (round-3 counters:
// 19 % VALU issue, 66 % of the wave cycles waiting).  FX (fx send bus) is a template parameter: its two accumulators cost 16 registers
// that the prefetch needs (123 of 128 before).
template <bool FAST, bool FX>
__device__ __forceinline__ void apply_tracks_body(const TrackApplyArgs& a, int b, int blk) {
    __shared__ float lds[8];
    const int chunk = blk * kWG + threadIdx.x;
    const int64_t i0 = (int64_t)chunk * CC;
    float accL[CC], accR[CC], fxL[FX ? CC : 1], fxR[FX ? CC : 1];
#pragma unroll
    for (int i = 0; i < CC; ++i) accL[i] = accR[i] = 0.0f;
    if (FX) {
#pragma unroll
        for (int i = 0; i < CC; ++i) fxL[i] = fxR[i] = 0.0f;
    }
    float xn[CC], xdn[CC];  // the NEXT track's samples (comp_on: at i0 and at i0 - lookahead)
    {
        const float* u0 = a.u + (int64_t)(b * a.T) * a.stride;
        LD8<FAST>(u0, i0, a.n, xn);
        if (a.comp_on) LD8S<FAST>(u0, i0 - a.lookahead, a.n, xdn);
    }
    for (int t = 0; t < a.T; ++t) {
        const int row = b * a.T + t;
        const float* rc = a.rc + (int64_t)row * RC_STRIDE;
        const float pl = rc[RC_PANL], pr = rc[RC_PANR];
        const float sl = FX ? pl * rc[RC_SEND] : 0.0f, sr = FX ? pr * rc[RC_SEND] : 0.0f;  // fx send bus: sum_t send_t * panned track
        float y[CC], x[CC], xd[CC];
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            x[i] = xn[i];
            xd[i] = xdn[i];
        }
        if (t + 1 < a.T) {
            const float* un = a.u + (int64_t)(row + 1) * a.stride;
            LD8<FAST>(un, i0, a.n, xn);
            if (a.comp_on) LD8S<FAST>(un, i0 - a.lookahead, a.n, xdn);
        }
        if (a.comp_on) {
            const CompK k = load_comp(rc);
            float g[CC];
            float z = 0.0f;
#pragma unroll
            for (int i = 0; i < CC; ++i) {
                float d;
                g[i] = k.oma * gain_computer(x[i], k, d);
                z = fmaf(k.alpha, z, g[i]);
            }
            const float ac = rc[RC_ALPHA_C], l2a = rc[RC_LOG2A_C];
            const float S = block_carry<false>(a.s0 + (int64_t)row * gridDim.x, blk, gridDim.x, l2a, lds, threadIdx.x);
            float s = block_enter<false>(z, ac, l2a, S, lds, threadIdx.x);
#pragma unroll
            for (int i = 0; i < CC; ++i) {
                s = fmaf(k.alpha, s, g[i]);
                g[i] = s;
                y[i] = xd[i] * lin_gain(s, k);
            }
            if (a.gs) ST8<FAST>(a.gs + (int64_t)row * a.stride, i0, a.n, g);
        } else {
#pragma unroll
            for (int i = 0; i < CC; ++i) y[i] = x[i];
        }
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            accL[i] = fmaf(pl, y[i], accL[i]);
            accR[i] = fmaf(pr, y[i], accR[i]);
        }
        if (FX) {
#pragma unroll
            for (int i = 0; i < CC; ++i) {
                fxL[i] = fmaf(sl, y[i], fxL[i]);
                fxR[i] = fmaf(sr, y[i], fxR[i]);
            }
        }
        if (a.mixed) {
            float ml[CC], mr[CC];
#pragma unroll
            for (int i = 0; i < CC; ++i) {
                ml[i] = pl * y[i];
                mr[i] = pr * y[i];
            }
            ST8<FAST>(a.mixed + (((int64_t)b * 2 + 0) * a.T + t) * a.n, i0, a.n, ml);
            ST8<FAST>(a.mixed + (((int64_t)b * 2 + 1) * a.T + t) * a.n, i0, a.n, mr);
        }
    }
    ST8<FAST>(a.bus + ((int64_t)b * 2 + 0) * a.bus_stride, i0, a.n, accL);
    ST8<FAST>(a.bus + ((int64_t)b * 2 + 1) * a.bus_stride, i0, a.n, accR);
    if (FX) {  // (bs, 2, stride) rows of the workspace: always 16-byte aligned
        ST8<FAST>(a.fx + ((int64_t)b * 2 + 0) * a.stride, i0, a.n, fxL);
        ST8<FAST>(a.fx + ((int64_t)b * 2 + 1) * a.stride, i0, a.n, fxR);
    }
}
__device__ __forceinline__ bool block_interior(int64_t n, int lookahead, int aligned, int blk = -1) {
    const int64_t lo = (int64_t)(blk < 0 ? (int)blockIdx.x : blk) * kWG * CC, hi = lo + (int64_t)kWG * CC;
    return aligned && lo - lookahead >= 0 && hi + lookahead <= n;
}
template <bool FX>
__global__ __launch_bounds__(kWG) void k_apply_tracks(TrackApplyArgs a) {
    // consecutive blocks of one mix on one XCD (mst_common.h: row_block_xcd): the look-ahead read of block b (samples 2048 earlier) is what
    // block b - 1 has just streamed through the same L2 - on the plain walk it was a second trip over the fabric for the whole of u
    int b, blk;
    row_block_xcd(b, blk);
    if (block_interior(a.n, a.lookahead, a.aligned, blk)) apply_tracks_body<true, FX>(a, b, blk);
    else apply_tracks_body<false, FX>(a, b, blk);
}

// ---- forward: master bus.  grid (nblk, bs).  out = delay(v) * G * gout  (stereo-linked)
template <bool FAST>
__device__ __forceinline__ void apply_master_body(const MasterApplyArgs& a, int b, int blk) {
    __shared__ float lds[8];
    const int chunk = blk * kWG + threadIdx.x;
    const int64_t i0 = (int64_t)chunk * CC;
    const float* rc = a.rc + (int64_t)b * RC_STRIDE;
    const float gout = rc[RC_PANL];
    const float* v0 = a.v + (int64_t)(b * 2) * a.stride;
    const float* v1 = v0 + a.stride;
    float yl[CC], yr[CC];
    if (a.comp_on) {
        const CompK k = load_comp(rc);
        float l[CC], r[CC], g[CC];
        LD8<FAST>(v0, i0, a.n, l);
        LD8<FAST>(v1, i0, a.n, r);
        float z = 0.0f;
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            float d;
            g[i] = k.oma * gain_computer(l[i] + r[i], k, d);
            z = fmaf(k.alpha, z, g[i]);
        }
        const float ac = rc[RC_ALPHA_C], l2a = rc[RC_LOG2A_C];
        // a.gran (no zero-state launch in front): this block's aggregate is published here, the earlier blocks' are picked up as they appear
        gran_t* gr = a.gran ? a.gran + (int64_t)b * gridDim.x : nullptr;
        if (gr) {
            const float agg = block_aggregate<false>(z, l2a, lds, threadIdx.x);
            if (threadIdx.x == 0) gran_publish(gr + blk, a.gran_near, agg);
        }
        LD8S<FAST>(v0, i0 - a.lookahead, a.n, yl);  // requested before the wait for the other blocks
        LD8S<FAST>(v1, i0 - a.lookahead, a.n, yr);
        const float S = gr ? block_carry_g<false>(gr, a.gran_near, carry_peek<false>(gr, a.gran_near, blk, gridDim.x, threadIdx.x), blk, gridDim.x, l2a, lds, threadIdx.x, a.status)
                           : block_carry<false>(a.s0 + (int64_t)b * gridDim.x, blk, gridDim.x, l2a, lds, threadIdx.x);
        float s = block_enter<false>(z, ac, l2a, S, lds, threadIdx.x);
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            s = fmaf(k.alpha, s, g[i]);
            g[i] = s;
            const float G = lin_gain(s, k) * gout;
            yl[i] *= G;
            yr[i] *= G;
        }
        if (a.gs) ST8<FAST>(a.gs + (int64_t)b * a.stride, i0, a.n, g);
    } else {
        LD8<FAST>(v0, i0, a.n, yl);
        LD8<FAST>(v1, i0, a.n, yr);
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            yl[i] *= gout;
            yr[i] *= gout;
        }
    }
    ST8<FAST>(a.out + ((int64_t)b * 2 + 0) * a.out_stride, i0, a.n, yl);
    ST8<FAST>(a.out + ((int64_t)b * 2 + 1) * a.out_stride, i0, a.n, yr);
}
__global__ __launch_bounds__(kWG) void k_apply_master(MasterApplyArgs a) {
    int b = blockIdx.y, blk = blockIdx.x;
    if (a.gran) row_block_xcd(b, blk);  // the blocks of one mix on one XCD, earlier blocks dispatched first (mst_common.h)
    if (block_interior(a.n, a.lookahead, a.aligned, blk)) apply_master_body<true>(a, b, blk);
    else apply_master_body<false>(a, b, blk);
}

// ---- backward ------------------------------------------------------------------------------------
// upstream cotangent of the compressor output y for 8 samples starting at i (may run past either end)
template <bool MASTER, bool FAST>
__device__ __forceinline__ void load_gy(const CompBwdArgs& a, int row, const float* rc, int64_t i, float* gl, float* gr) {
    // raw upstream cotangents per stereo channel: grad_mix (MASTER) or grad_bus (+ grad_mixed_tracks)
    const int b = MASTER ? row : row / a.T;
    float l[CC], r[CC];
    LD8S<FAST>(a.gup + ((int64_t)b * 2 + 0) * a.gup_stride, i, a.n, l);
    LD8S<FAST>(a.gup + ((int64_t)b * 2 + 1) * a.gup_stride, i, a.n, r);
    if (!MASTER && a.gmixed) {
        const int t = row % a.T;
        float ml[CC], mr[CC];
        LD8S<FAST>(a.gmixed + (((int64_t)b * 2 + 0) * a.T + t) * a.n, i, a.n, ml);
        LD8S<FAST>(a.gmixed + (((int64_t)b * 2 + 1) * a.T + t) * a.n, i, a.n, mr);
#pragma unroll
        for (int q = 0; q < CC; ++q) {
            l[q] += ml[q];
            r[q] += mr[q];
        }
    }
    if (!MASTER && a.gfx) {  // the panned track also feeds the fx send bus with gain `send`
        const float send = rc[RC_SEND];
        float fl[CC], fr[CC];
        LD8S<FAST>(a.gfx + ((int64_t)b * 2 + 0) * a.gfx_stride, i, a.n, fl);
        LD8S<FAST>(a.gfx + ((int64_t)b * 2 + 1) * a.gfx_stride, i, a.n, fr);
#pragma unroll
        for (int q = 0; q < CC; ++q) {
            l[q] = fmaf(send, fl[q], l[q]);
            r[q] = fmaf(send, fr[q], r[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < CC; ++q) {
        gl[q] = l[q];
        gr[q] = r[q];
    }
}

// ---- coefficient-gradient sums of the block, formed where du and u are in registers ------------------------------------------
// The all-pole bank 1/A_k, b0/B_k on u from the saved chunk-entry states and five inner products with the
// cotangent per section, on this workgroup's 2048 samples = 32 chunks of 64: the block's du and u go to LDS in the chunk-per-row
// layout, lane (section s = tid >> 5, chunk c = tid & 31) walks its chunk with ONE section, the 32
// chunk lanes of a section meet in a half-wave shuffle sum.  192 of the 256 lanes work; the cotangent du crosses HBM only if
// someone downstream wants it, u is not fetched a second time.
#ifndef MST_CG_PITCH
#define MST_CG_PITCH (kEqChunk + 4)
#endif
constexpr int kCgPitch = MST_CG_PITCH, kCgChunks = kWG * CC / kEqChunk, kCgTile = kCgChunks * kCgPitch;
static_assert((kCgChunks == 32 || kCgChunks == 8) && kSections * kCgChunks <= kWG, "one section x kCgChunks chunks per lane group");
// the four all-pole states entering this lane's (section, chunk) walk
struct CgStates { float wa1, wa2, wb1, wb2; };
__device__ __forceinline__ int cg_chunk_of(int tid) { return kCgChunks == 32 ? (tid & 31) : tid % kCgChunks; }
__device__ __forceinline__ CgStates coefgrad_states(const CompBwdArgs& a, int blk, int sig) {
    const int tid = threadIdx.x, s = tid / kCgChunks, c = cg_chunk_of(tid);
    CgStates w = {0.f, 0.f, 0.f, 0.f};
    if (s < kSections) {
        const int64_t base = ((int64_t)sig * 24 + 4 * s) * a.ap_nc_pad + (int64_t)blk * kCgChunks + c;
        w.wa1 = a.ap_s0[base];
        w.wa2 = a.ap_s0[base + a.ap_nc_pad];
        w.wb1 = a.ap_s0[base + 2 * (int64_t)a.ap_nc_pad];
        w.wb2 = a.ap_s0[base + 3 * (int64_t)a.ap_nc_pad];
    }
    return w;
}
template <bool FAST>
__device__ __forceinline__ void coefgrad_fused(const CompBwdArgs& a, int blk, int sig, const float* __restrict__ rc, int64_t i0, const float* xu,
                                               const float* du, float* __restrict__ cg_u, float* __restrict__ cg_g) {
    const int tid = threadIdx.x;
    {
        const int c = tid >> 3, off = (tid & 7) * CC;  // 8 lanes x 8 samples = one chunk
        float g[CC];
#pragma unroll
        for (int i = 0; i < CC; ++i) g[i] = (FAST || i0 + i < a.n) ? du[i] : 0.0f;
        // chunk row image: sample 8 j + 4 h + e sits at float h 32 + 4 j + e (j = lane of the chunk, h = half of its eight samples), so that
        // the eight lanes of a ds_write_b128 group cover 32 consecutive banks (sample order 8 j + e put lanes j and j + 4 on the same banks:
        // a 2-way conflict on every store of the transposition - round-3 counters: 43 % of this kernel's LDS cycles)
        (void)off;
        float* pu = &cg_u[c * kCgPitch + 4 * (tid & 7)];
        float* pg = &cg_g[c * kCgPitch + 4 * (tid & 7)];
        *reinterpret_cast<float4*>(pu) = make_float4(xu[0], xu[1], xu[2], xu[3]);
        *reinterpret_cast<float4*>(pu + 32) = make_float4(xu[4], xu[5], xu[6], xu[7]);
        *reinterpret_cast<float4*>(pg) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(pg + 32) = make_float4(g[4], g[5], g[6], g[7]);
    }
    if (kCompWaves > 1) lds_barrier();
    else wave_lds_sync();
    const int s = tid / kCgChunks, c = cg_chunk_of(tid);
    if (s < kSections) {
        const float ka1 = rc[RC_SOS + 5 * s + 3], ka2 = rc[RC_SOS + 5 * s + 4];
        const float kc1 = rc[RC_AP + 3 * s], kc2 = rc[RC_AP + 3 * s + 1], kib0 = rc[RC_AP + 3 * s + 2];
        const CgStates w0 = coefgrad_states(a, blk, sig);
        const float wa1 = w0.wa1, wa2 = w0.wa2, wb1 = w0.wb1, wb2 = w0.wb2;
        // The two recurrences (1 / B_s and 1 / A_s driven by the same input) and the lag-1 / lag-2 inner products are the same arithmetic
        // on two values: held as float pairs they take one packed instruction each (v_pk_fma_f32) - five instructions per sample
        // instead of nine.  Lane x of a pair = the 1 / B_s side (numerator sums), lane y = the 1 / A_s side (its sums enter negated).
        float db0 = 0.f, db1, db2, da1, da2;
        const float* mu = &cg_u[c * kCgPitch];
        const float* mg = &cg_g[c * kCgPitch];
        f2 w1 = {wb1, wa1}, w2 = {wb2, wa2}, acc1 = {0.f, 0.f}, acc2 = {0.f, 0.f};
        const f2 nk1 = {-kc1, -ka1}, nk2 = {-kc2, -ka2};
#pragma unroll 2
        for (int i4 = 0; i4 < kEqChunk; i4 += 4) {
            const int at = ((i4 >> 2) & 1) * 32 + (i4 >> 3) * 4;  // samples i4 .. i4 + 3 in the row image (see the stores above)
            const float4 xv = *reinterpret_cast<const float4*>(&mu[at]);
            const float4 gv = *reinterpret_cast<const float4*>(&mg[at]);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f2 xx = {xs[t], xs[t]}, gg = {gs[t], -gs[t]};
                const f2 wn = f2_fma(nk2, w2, f2_fma(nk1, w1, xx));
                db0 = fmaf(gs[t], wn.x, db0);
                acc1 = f2_fma(gg, w1, acc1);
                acc2 = f2_fma(gg, w2, acc2);
                w2 = w1;
                w1 = wn;
            }
        }
        db1 = acc1.x; da1 = acc1.y; db2 = acc2.x; da2 = acc2.y;
        float acc[5] = {db0 * kib0, db1 * kib0, db2 * kib0, da1, da2};
        // sum over the 32 chunk lanes of the section (one half wave), fixed order: four DPP row shifts leave every 16-lane row's total in
        // its last lane, row_bcast:15 adds row 0's into row 1 (row 2's into row 3) - lane 31 / 63 holds the half-wave sum.  (The five
        // ds_bpermute levels this replaces were 50 of the kernel's 64 LDS-crossbar round trips and what rocprof reported as 40 % "bank
        // conflict" cycles: the LDS images themselves are conflict-free, tools/lds_conflicts.py.)
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            float v = acc[i];
            if (kCgChunks == 32) {
                v = dpp_add<0x111, 0xf>(v);
                v = dpp_add<0x112, 0xf>(v);
                v = dpp_add<0x114, 0xf>(v);
                v = dpp_add<0x118, 0xf>(v);
                v = dpp_add<0x142, 0xa>(v);
            } else {  // eight chunk lanes per section: xor 1, xor 2 (quad permutes), then the other quad of the 8-lane group (row_half_mirror)
                v = dpp_add<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
                v = dpp_add<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
                v = dpp_add<0x141, 0xf>(v);  // row_half_mirror
            }
            acc[i] = v;
        }
        if ((tid % kCgChunks) == kCgChunks - 1) {
            float* o = a.ep + ((int64_t)sig * gridDim.x + blk) * EP_COUNT + 5 * s;
#pragma unroll
            for (int i = 0; i < 5; ++i) o[i] = acc[i];
        }
    }
    if (kCompWaves > 1) lds_barrier();  // red[] below and the next use of the tiles
    else wave_lds_sync();
}

// FXS: the fx send bus is on (tracks only) - its cotangent rows are read and the send-gain sum is formed
template <bool MASTER, bool FAST, bool FXS>
__device__ __forceinline__ void comp_bwd_run_body(const CompBwdArgs& a, int row, int blk, float* __restrict__ cg_u, float* __restrict__ cg_g) {
    constexpr int NCH = MASTER ? 2 : 1;
    __shared__ float red[kCompWaves > 1 ? kCompWaves : 1][CP_COUNT];  // red[0] doubles as the 8-float scan scratch
    const int tid = threadIdx.x, chunk = blk * kWG + tid;
    const int64_t i0 = (int64_t)chunk * CC;
    const float* rc = a.rc + (int64_t)row * RC_STRIDE;
    const float* u0 = a.u + (int64_t)(row * NCH) * a.stride;
    const float* u1 = u0 + a.stride;
    float p[CP_COUNT];
#pragma unroll
    for (int i = 0; i < CP_COUNT; ++i) p[i] = 0.0f;
    float gl[CC], gr[CC], du0[CC], du1[CC];
    float xu[CC], xu1[MASTER ? CC : 1];  // the compressor input of this lane's samples, kept for the fused coefficient-gradient pass
    CBR_STAMP(0);
    load_gy<MASTER, FAST>(a, row, rc, i0, gl, gr);
    const float pl = rc[RC_PANL], pr = rc[RC_PANR];  // master: both = output-fader gain
    // cotangent of the fx send gain: sum_n (pl fL + pr fR)[n] y[n]  (fL, fR = cotangent of the send bus)
    float fsum[FXS ? CC : 1];
    if (FXS) {
        const int bb = row / a.T;
        float fl[CC], fr[CC];
        LD8S<FAST>(a.gfx + ((int64_t)bb * 2 + 0) * a.gfx_stride, i0, a.n, fl);
        LD8S<FAST>(a.gfx + ((int64_t)bb * 2 + 1) * a.gfx_stride, i0, a.n, fr);
#pragma unroll
        for (int i = 0; i < CC; ++i) fsum[i] = pl * fl[i] + pr * fr[i];
    }

    if (a.comp_on) {
        const CompK k = load_comp(rc);
        float x0[CC], x1[CC], xd0[CC], xd1[CC], g[CC];
        // what the adjoint smoother's zero-state value needs comes first: with a.gran the block's aggregate is published as early as
        // possible (no zero-state launch) and the later blocks' aggregates are awaited only after every other load has been requested
        LD8S<FAST>(u0, i0 - a.lookahead, a.n, xd0);
        if (MASTER) LD8S<FAST>(u1, i0 - a.lookahead, a.n, xd1);
        LD8<FAST>(a.gs + (int64_t)row * a.stride, i0, a.n, g);
        // The adjoint smoother's state enters every q-dependent quantity as  zero-state part + Q x homogeneous part  (q is linear in the
        // state Q entering the lane's chunk); both parts are formed BEFORE the other blocks' aggregates are awaited, behind the wait are
        // one multiply-add per sample and per sum
        float dgsv[CC];
        float zq = 0.0f;
#pragma unroll
        for (int i = CC - 1; i >= 0; --i) {
            const float Gi = lin_gain(g[i], k);
            const float dot = MASTER ? pl * (gl[i] * xd0[i] + gr[i] * xd1[i]) : (pl * gl[i] + pr * gr[i]) * xd0[i];
            dgsv[i] = (FAST || i0 + i < a.n) ? dot * Gi * kLn10Over20 : 0.0f;
            zq = fmaf(k.alpha, zq, dgsv[i]);
            // the pan / make-up / send sums need exactly these operands: formed here, the upstream cotangents and the delayed input
            // are dead before the static-curve loop starts
            if (FAST || i0 + i < a.n) {
                p[CP_MAKEUP] += dgsv[i];
                if (MASTER) {
                    p[CP_PANL] = fmaf(gl[i] * xd0[i] + gr[i] * xd1[i], Gi, p[CP_PANL]);  // output-fader gain: sum(grad_mix * out_before_fader)
                } else {
                    const float yv = xd0[i] * Gi;
                    p[CP_PANL] = fmaf(gl[i], yv, p[CP_PANL]);
                    p[CP_PANR] = fmaf(gr[i], yv, p[CP_PANR]);
                    if (FXS) p[CP_SEND] = fmaf(fsum[i], yv, p[CP_SEND]);
                }
            }
        }
        const float ac = rc[RC_ALPHA_C], l2a = rc[RC_LOG2A_C];
        gran_t* gq = a.gran ? a.gran + (int64_t)row * gridDim.x : nullptr;
        CBR_STAMP(1);
        if (gq) {
            const float agg = block_aggregate<true>(zq, l2a, red[0], tid);
            if (tid == 0) gran_publish(gq + blk, a.gran_near, agg);
        }
        CBR_STAMP(2);
        // look-ahead branch: du[i] += gy[i+L] * G[i+L].  Folded to one (two: master) value per sample right after the loads -
        // three arrays less are alive across the block scan (the kernel ran at 152 registers = 3 waves per SIMD)
        float fwd0[CC], fwd1[MASTER ? CC : 1];
        {
            float gF[CC], glF[CC], grF[CC];
            LD8S<FAST>(a.gs + (int64_t)row * a.stride, i0 + a.lookahead, a.n, gF);
            load_gy<MASTER, FAST>(a, row, rc, i0 + a.lookahead, glF, grF);
#pragma unroll
            for (int i = 0; i < CC; ++i) {
                const bool liveF = FAST || i0 + i + a.lookahead < a.n;
                const float GF = lin_gain(gF[i], k);
                fwd0[i] = liveF ? (MASTER ? pl * glF[i] : pl * glF[i] + pr * grF[i]) * GF : 0.0f;
                if (MASTER) fwd1[i] = liveF ? pr * grF[i] * GF : 0.0f;
            }
        }
        CBR_STAMP(3);
        LD8<FAST>(u0, i0, a.n, x0);
        if (MASTER) LD8<FAST>(u1, i0, a.n, x1);
        const float g_prev0 = (i0 > 0 && i0 - 1 < a.n) ? a.gs[(int64_t)row * a.stride + i0 - 1] : 0.0f;
#pragma unroll
        for (int i = 0; i < CC; ++i) xu[i] = x0[i];
        if (MASTER) {
#pragma unroll
            for (int i = 0; i < CC; ++i) xu1[i] = x1[i];
        }
        // scheduling fences between the phases and between the samples of the static-curve loop: unfenced the compiler interleaves all
        // eight samples and needs 172 registers
        __builtin_amdgcn_sched_barrier(0);
        // state entering this lane's chunk = Q0 + W S (S = state entering the block, known after the wait)
        float Q0 = 0.0f, W = 0.0f;
        block_enter_split<true>(zq, ac, l2a, red[0], tid, Q0, W);
        const gran_t peek = gq ? carry_peek<true>(gq, a.gran_near, blk, gridDim.x, tid) : 0ull;
        CBR_STAMP(4);
        // q[i] = zs[i] + pw[i] Q with zs the zero-entry recurrence over this lane's samples and pw[i] = alpha^(CC - i):
        //   alpha += q A;  kappa += oma q Fv;  thr -= oma q Kp;  knee += oma q Kw;  du = oma q E + look-ahead branch
        // pairs (zero-state part, homogeneous part): one packed multiply-add per sum and sample
        f2 zp = {0.0f, 1.0f}, sA = {0.f, 0.f}, sF = {0.f, 0.f}, sP = {0.f, 0.f}, sW = {0.f, 0.f};
        const float kinvw = k.kappa * k.invw, kw2 = k.kappa * k.inv2w * k.invw, ke = k.oma * 8.685889638065035f;
        float db[CC];  // du0 / du1 hold the zero-state part until Q is known
#pragma unroll
        for (int i = CC - 1; i >= 0; --i) {
            const bool live = FAST || i0 + i < a.n;
            const float side = MASTER ? x0[i] + x1[i] : x0[i];
            // static curve and its derivatives (mst_compdev.h: curve_f): f, kappa df/dd, kappa df/dknee
            float tc;
            const float fval = curve_f(curve_t(side, k), k, tc);
            const float gprev = (i > 0) ? g[i - 1] : g_prev0;
            const float kp = tc * kinvw;
            const float cKw = tc * (k.knee - tc) * kw2;
            // beyond the row's end the guarded loads return 0: side = 0 gives tc = 0 (f and both derivatives vanish) and the clamp below
            // kills the side chain; only g[i-1] - g_c has to be masked
            const float cA = live ? fmaf(-k.kappa, fval, gprev) : 0.0f;
            // side chain: d x_db / d side = (20/ln10) / side, clamp kills it below eps
            const float cE = (fabsf(side) >= kCompEps) ? kp * ke * __builtin_amdgcn_rcpf(side) : 0.0f;
            zp.x = fmaf(k.alpha, zp.x, dgsv[i]);  // zs: zero-entry recurrence
            zp.y *= k.alpha;                      // pw = alpha^(CC - i)
            sA = f2_fma(zp, f2{cA, cA}, sA);
            sF = f2_fma(zp, f2{fval, fval}, sF);
            sP = f2_fma(zp, f2{kp, kp}, sP);
            sW = f2_fma(zp, f2{cKw, cKw}, sW);
            du0[i] = fmaf(zp.x, cE, fwd0[i]);
            if (MASTER) du1[i] = fmaf(zp.x, cE, fwd1[i]);
            db[i] = zp.y * cE;
            // the loop is pinned in front of the granule wait (tools/cbr_timeline.py showed it sunk BEHIND the wait, into the block that
            // uses its results: the wait then overlapped nothing)
            pin(du0[i]);
            if (MASTER) pin(du1[i]);
            pin(db[i]);
            __builtin_amdgcn_sched_barrier(0);
        }
        pin2(sA);
        pin2(sF);
        pin2(sP);
        pin2(sW);
        CBR_STAMP(5);
        const float S = gq ? block_carry_g<true>(gq, a.gran_near, peek, blk, gridDim.x, l2a, red[0], tid, a.status)
                           : block_carry<true>(a.s0 + (int64_t)row * gridDim.x, blk, gridDim.x, l2a, red[0], tid);
        CBR_STAMP(6);
        const float Q = fmaf(W, S, Q0);
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            du0[i] = fmaf(Q, db[i], du0[i]);
            if (MASTER) du1[i] = fmaf(Q, db[i], du1[i]);
        }
        p[CP_ALPHA] = fmaf(Q, sA.y, sA.x);
        p[CP_KAPPA] = k.oma * fmaf(Q, sF.y, sF.x);
        p[CP_THR] = -k.oma * fmaf(Q, sP.y, sP.x);
        p[CP_KNEE] = k.oma * fmaf(Q, sW.y, sW.x);
    } else {
        float x0[CC], x1[CC];
        LD8<FAST>(u0, i0, a.n, x0);
        if (MASTER) LD8<FAST>(u1, i0, a.n, x1);
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            xu[i] = x0[i];
            if (MASTER) xu1[i] = x1[i];
        }
#pragma unroll
        for (int i = 0; i < CC; ++i) {
            du0[i] = MASTER ? pl * gl[i] : pl * gl[i] + pr * gr[i];
            if (MASTER) du1[i] = pr * gr[i];
            if (i0 + i < a.n) {
                if (MASTER) p[CP_PANL] = fmaf(gl[i], x0[i], fmaf(gr[i], x1[i], p[CP_PANL]));
                else {
                    p[CP_PANL] = fmaf(gl[i], x0[i], p[CP_PANL]);
                    p[CP_PANR] = fmaf(gr[i], x0[i], p[CP_PANR]);
                    if (FXS) p[CP_SEND] = fmaf(fsum[i], x0[i], p[CP_SEND]);
                }
            }
        }
    }
    if (a.du) {
        ST8<FAST>(a.du + (int64_t)(row * NCH) * a.stride, i0, a.n, du0);
        if (MASTER) ST8<FAST>(a.du + (int64_t)(row * NCH + 1) * a.stride, i0, a.n, du1);
    }
    CBR_STAMP(7);
    if (a.ep) {  // signal rows: tracks = row, master = 2 row + channel
        coefgrad_fused<FAST>(a, blk, row * NCH, rc, i0, xu, du0, cg_u, cg_g);
        if (MASTER) coefgrad_fused<FAST>(a, blk, row * NCH + 1, rc, i0, xu1, du1, cg_u, cg_g);
    }

    CBR_STAMP(8);
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < CP_COUNT; ++i) {
        const float v = wave_sum(p[i]);
        if (lane == 0) red[wave][i] = v;
    }
    if (kCompWaves > 1) lds_barrier();
    else wave_lds_sync();
    if (tid < CP_COUNT) {
        float t = 0.0f;
        if constexpr (kCompWaves == 4) t = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        else
            for (int w = 0; w < kCompWaves; ++w) t += red[w][tid];
        a.part[((int64_t)row * gridDim.x + blk) * CP_COUNT + tid] = t;
    }
    CBR_STAMP(9);
}
#ifndef MST_COMP_BWD_W
#define MST_COMP_BWD_W 1  // min waves per SIMD asked of the compressor backward (tracks with the fx send bus)
#endif
template <bool MASTER, bool FXS = false>
#ifndef MST_COMP_BWD_WT
#define MST_COMP_BWD_WT 4
#endif
#ifndef MST_COMP_BWD_WM
#define MST_COMP_BWD_WM 4  // master rows (round 6): 137 registers uncapped = three waves per SIMD = 1.33 rounds of its 1024 workgroups at cfg #2;
                           // capped at 128 (8 spilled, also in the path with the coefficient-gradient walks that cfg #2 does not take) one round: 18.5 -> 17.9 us
#endif
__global__ __launch_bounds__(kWG, (!MASTER && !FXS) ? MST_COMP_BWD_WT : (MASTER ? MST_COMP_BWD_WM : MST_COMP_BWD_W)) void k_comp_bwd_run(CompBwdArgs a) {  // tracks without fx: 130 registers uncapped, two short of four waves per SIMD
    __shared__ __attribute__((aligned(16))) float cg_u[kCgTile], cg_g[kCgTile];  // one copy for both bodies
    // a.gran: the blocks a workgroup waits for (LATER in time: the adjoint smoother runs backwards) must have been dispatched before
    // it, so the grid walks the row from its end
    int row = blockIdx.y, blk = blockIdx.x;
    const int extra = MASTER ? 0 : a.cg2_rows, main_rows = (int)gridDim.y - extra;
    // Coefficient-gradient-only rows (one channel of a master bus each; its compressor adjoint ran in the master launch) are light
    // workgroups.  Behind the track rows they were a 21 us tail of half-empty rounds; they come FIRST in the grid (+13 us; interleaved
    // with the track workgroups they measured worse).
    if (!MASTER && row < extra) {
        CBR_STAMP(10);
        const int j = row;
        const int64_t i0 = ((int64_t)blk * kWG + threadIdx.x) * CC;
        const bool fast = a.aligned && (int64_t)(blk + 1) * kWG * CC <= a.n;
        float xu[CC], du[CC];
        if (fast) {
            ld8f(a.cg2_u + (int64_t)j * a.stride, i0, xu);
            ld8f(a.cg2_du + (int64_t)j * a.stride, i0, du);
            coefgrad_fused<true>(a, blk, main_rows + j, a.cg2_rc + (int64_t)(j >> 1) * RC_STRIDE, i0, xu, du, cg_u, cg_g);
        } else {
            ld8(a.cg2_u + (int64_t)j * a.stride, i0, a.n, xu);
            ld8(a.cg2_du + (int64_t)j * a.stride, i0, a.n, du);
            coefgrad_fused<false>(a, blk, main_rows + j, a.cg2_rc + (int64_t)(j >> 1) * RC_STRIDE, i0, xu, du, cg_u, cg_g);
        }
        CBR_STAMP(11);
        return;
    }
    if (a.gran) {
        row_block_xcd(row, blk, MASTER ? 1 : a.T, main_rows, extra);  // the blocks of one row - and the tracks of one mix - on one XCD (mst_common.h)
        blk = gridDim.x - 1 - blk;
    } else {
        row -= extra;
    }
    if (block_interior(a.n, a.lookahead, a.aligned, blk)) comp_bwd_run_body<MASTER, true, FXS>(a, row, blk, cg_u, cg_g);
    else comp_bwd_run_body<MASTER, false, FXS>(a, row, blk, cg_u, cg_g);
}

// A mix-wise form of the tracks backward (k_comp_bwd_mix: one workgroup per mix and block, looping over the mix's tracks) was built and
// measured slower, 119 us against 97-99 us; it is not in the tree any more (DESIGN 12.1 has the measurements and the last commit with it).

// ---- launch helpers ---------------------------------------------------------------------------------
void launch_apply_tracks(const TrackApplyArgs& a, int bs, hipStream_t stream) {
    if (a.fx) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_apply_tracks<true>), dim3(a.nc_pad / kWG, bs), dim3(kWG), 0, stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_apply_tracks<false>), dim3(a.nc_pad / kWG, bs), dim3(kWG), 0, stream, a);
}
void launch_apply_master(const MasterApplyArgs& a, int bs, hipStream_t stream) {
    hipLaunchKernelGGL(k_apply_master, dim3(a.nc_pad / kWG, bs), dim3(kWG), 0, stream, a);
}
void launch_comp_bwd(bool master, const CompBwdArgs& a, int rows, hipStream_t stream) {
    dim3 grid(a.nc_pad / kWG, rows + (master ? 0 : a.cg2_rows)), block(kWG);
    if (master) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_comp_bwd_run<true>), grid, block, 0, stream, a);
    else if (a.gfx) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_comp_bwd_run<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_comp_bwd_run<false>), grid, block, 0, stream, a);
}

}  // namespace mst
