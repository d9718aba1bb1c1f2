// mst_sections.hip - picks the sections a sectioned fit (mst.online.optimize_sections) is run on, from the windowed loudness of the
// tracks and of their mix (mst_loudness_windows): greedy cover, so that every track plays in some section.
//
// The rule (include/diffmst_hip.h states it; tests/sections_ref.py restates it in numpy):
//   active[t][w] = track_lufs[t][w] >= track_floor[t];  eligible[w] = mix_lufs[w] >= mix_floor and some track is active in w
//   round r takes, among the eligible windows at least min_gap away from every window taken so far, the one with the largest
//   (tracks active in w and not yet covered, tracks active in w, mix_lufs[w], -w), and marks its active tracks covered
// One workgroup, one launch.  A lane owns the windows lane, lane + 512, ... and keeps their active sets as bit masks in registers
// (up to 8 windows x 256 tracks), so a round is a popcount per window and one 64-bit maximum over the workgroup: the four-part
// key is packed into one integer, (new << 53) | (act << 44) | (order-preserving bits of mix_lufs << 12) | (4095 - w).
#include "mst_common.h"

namespace mst {

constexpr int kPickThreads = 512;
constexpr int kPickWaves = kPickThreads / 64;
constexpr int kPickPer = 8;                                 // windows per lane
constexpr int kPickWords = MST_PICK_MAX_TRACKS / 64;        // 64-bit words of an active set
static_assert(kPickThreads * kPickPer >= MST_LOUDNESS_MAX_BLOCKS, "every window has an owner");
static_assert(MST_PICK_MAX_TRACKS % 64 == 0 && MST_PICK_MAX_TRACKS < 512 && MST_LOUDNESS_MAX_BLOCKS < 4096, "fields of the key");

// bits of a float that compare as unsigned integers the way the floats compare (no NaN reaches this; -0 is made +0 first)
__device__ __forceinline__ uint32_t pick_ordered_bits(float v) {
    const uint32_t b = (uint32_t)__float_as_int(v + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the largest key of the workgroup, in every lane (0: no lane has a candidate)
__device__ __forceinline__ unsigned long long pick_block_max(unsigned long long key, unsigned long long* s_wave, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o > key ? o : key;
    }
    __syncthreads();  // the previous round's readers of s_wave are done
    if ((tid & 63) == 0) s_wave[tid >> 6] = key;
    __syncthreads();
    key = s_wave[0];
#pragma unroll
    for (int i = 1; i < kPickWaves; ++i) key = s_wave[i] > key ? s_wave[i] : key;
    return key;
}

__global__ __launch_bounds__(kPickThreads) void k_pick_sections(const float* __restrict__ track_lufs, const float* __restrict__ mix_lufs,
                                                                const float* __restrict__ track_floor, float mix_floor, int T, int NW,
                                                                int count, int min_gap, int32_t* __restrict__ windows,
                                                                uint8_t* __restrict__ active, uint8_t* __restrict__ covered) {
    __shared__ unsigned long long s_wave[kPickWaves], s_cov[kPickWords], s_sel[kPickWords];
    const int tid = threadIdx.x;
    unsigned long long mask[kPickPer][kPickWords];
    unsigned long long mixkey[kPickPer];  // the constant low part of a window's key, 0 for a window that can no longer be taken
#pragma unroll
    for (int k = 0; k < kPickPer; ++k) {
#pragma unroll
        for (int q = 0; q < kPickWords; ++q) mask[k][q] = 0ull;
    }
#pragma unroll
    for (int q = 0; q < kPickWords; ++q) {
        for (int tt = 0; tt < 64 && q * 64 + tt < T; ++tt) {
            const int t = q * 64 + tt;
            const float floor_t = track_floor[t];
#pragma unroll
            for (int k = 0; k < kPickPer; ++k) {
                const int w = tid + k * kPickThreads;
                if (w < NW && track_lufs[(int64_t)t * NW + w] >= floor_t) mask[k][q] |= 1ull << tt;  // NaN, -inf: not active
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPickPer; ++k) {
        const int w = tid + k * kPickThreads;
        int act = 0;
#pragma unroll
        for (int q = 0; q < kPickWords; ++q) act += __builtin_popcountll(mask[k][q]);
        mixkey[k] = 0ull;
        if (w < NW && act > 0) {
            const float m = mix_lufs[w];
            if (m >= mix_floor)
                mixkey[k] = ((unsigned long long)act << 44) | ((unsigned long long)pick_ordered_bits(m) << 12) | (unsigned long long)(4095 - w);
        }
    }
    if (tid < kPickWords) s_cov[tid] = 0ull;
    __syncthreads();

    int r = 0;
    for (; r < count; ++r) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int k = 0; k < kPickPer; ++k) {
            int fresh = 0;
#pragma unroll
            for (int q = 0; q < kPickWords; ++q) fresh += __builtin_popcountll(mask[k][q] & ~s_cov[q]);
            const unsigned long long key = mixkey[k] ? (((unsigned long long)fresh << 53) | mixkey[k]) : 0ull;
            best = key > best ? key : best;
        }
        best = pick_block_max(best, s_wave, tid);  // its barriers also order the reads of s_cov above before the update below
        if (best == 0ull) break;                   // the same value in every lane
        const int sel = 4095 - (int)(best & 4095ull);
        if (tid == sel % kPickThreads) {
#pragma unroll
            for (int k = 0; k < kPickPer; ++k) {
                if (k == sel / kPickThreads) {
#pragma unroll
                    for (int q = 0; q < kPickWords; ++q) {
                        s_sel[q] = mask[k][q];
                        s_cov[q] |= mask[k][q];
                    }
                }
            }
            windows[r] = sel;
        }
        __syncthreads();
        for (int t = tid; t < T; t += kPickThreads) active[(int64_t)r * T + t] = (uint8_t)((s_sel[t >> 6] >> (t & 63)) & 1ull);
#pragma unroll
        for (int k = 0; k < kPickPer; ++k) {
            const int d = tid + k * kPickThreads - sel;
            if ((d < 0 ? -d : d) < min_gap) mixkey[k] = 0ull;
        }
    }
    for (; r < count; ++r) {  // no candidate left
        if (tid == 0) windows[r] = -1;
        for (int t = tid; t < T; t += kPickThreads) active[(int64_t)r * T + t] = 0;
    }
    for (int t = tid; t < T; t += kPickThreads) covered[t] = (uint8_t)((s_cov[t >> 6] >> (t & 63)) & 1ull);
}

}  // namespace mst

using namespace mst;

extern "C" int mst_pick_sections(const float* track_lufs, const float* mix_lufs, const float* track_floor, float mix_floor,
                                 int32_t n_tracks, int32_t n_windows, int32_t count, int32_t min_gap, int32_t* windows,
                                 uint8_t* active, uint8_t* covered, void* stream) {
    if (!track_lufs || !mix_lufs || !track_floor || !windows || !active || !covered || n_tracks < 1 || n_tracks > MST_PICK_MAX_TRACKS ||
        n_windows < 1 || n_windows > MST_LOUDNESS_MAX_BLOCKS || count < 1 || count > MST_OPT_MAX_SECTIONS || min_gap < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pick_sections, dim3(1), dim3(kPickThreads), 0, (hipStream_t)stream, track_lufs, mix_lufs, track_floor,
                       mix_floor, (int)n_tracks, (int)n_windows, (int)count, (int)min_gap, windows, active, covered);
    return (int)hipGetLastError();
}
