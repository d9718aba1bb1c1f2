// mst_opt.hip - the bookkeeping of per-song mix optimisation (diffmst_hip/online.py; the loop of the reference's scripts/online.py:71-106)
// as ONE launch per iteration: chain dL/dp through the sigmoid, apply Adam to the logits, emit the next iteration's (0,1) parameters,
// append the loss terms to a device-side history and advance the step count - nothing of it passes through the host.
// PARITY UNPINNED: the arithmetic restates torch.optim.Adam (single-tensor path, defaults: no weight decay, no amsgrad) behind
// torch.sigmoid from torch's published source, operation by operation as the CPU kernels evaluate them:
//     g  = (dp (1 - p)) p                                   sigmoid_backward, with the p the console consumed
//     m  = m + w1 (g - m)              w1 = fp32(1 - b1)     exp_avg.lerp_(grad, 1 - beta1)  (the branch torch takes for w1 < 0.5)
//     v  = v b2 + (w2 g) g             w2 = fp32(1 - b2)     exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//     th = th + (s m) / (sqrt(v) / c2 + eps)                 s = fp32(-lr / (1 - b1^t)), c2 = fp32(sqrt(1 - b2^t)), both from float64
//     p  = 1 / (1 + exp(-th))
// Every rounding is written out: this unit is compiled with -ffp-contract=off (Makefile).
// A song has 27 T + 51 parameters, so the whole step is one workgroup that loops.  Its first pass looks at every gradient element and
// loss term; a workgroup-wide flag in LDS carries "something is not finite" to the second pass, which then leaves every coordinate
// alone (torch would spread the NaN through all of them).  Every lane reads and writes only the coordinates i = tid + k 256 < count of
// a segment; the history row is written by lane 0, 1 + n_terms floats.
// The `_best` kernels are the same body with three additions inside the same launch: lane 0 compares the loss sum with the
// best one in a second caller-owned block and publishes the verdict through LDS at the barrier the step has anyway; on an improvement
// every lane copies its coordinates of theta into that block BEFORE it updates them (the theta the loss was evaluated at); and an
// item whose wait count has reached `patience` is marked settled, after which its calls write their history row and nothing else.
#include <math.h>

#include "mst_common.h"

namespace mst {

constexpr int kOptWG = 256;
constexpr int kOptHdr = 16;               // int32 words in front of the moments (include/diffmst_hip.h)
constexpr int64_t kOptMaxParams = 1 << 20;  // per item
constexpr int kOptMaxItems = 1024;
constexpr int kBestHdr = 16;  // int32 words in front of the best logits (include/diffmst_hip.h)
constexpr int kBestSettled = 1, kBestImproved = 2;  // s_best below

// what the `_best` kernels take besides; `block` is NULL in the plain kernels, whose code has none of it (kBest = false)
struct OptBest {
    int32_t* block;   // this item's: header, best logits, best history row
    float min_delta;
    int32_t patience;
};

struct OptArgs {
    float* theta[MST_OPT_MAX_SEGMENTS];
    float* p[MST_OPT_MAX_SEGMENTS];
    const float* grad_p[MST_OPT_MAX_SEGMENTS];
    int32_t count[MST_OPT_MAX_SEGMENTS];
    int32_t n_segments;
    const float* term[MST_OPT_MAX_TERMS];
    int32_t n_terms;
    int32_t n_params;
};

__device__ __forceinline__ bool opt_finite(float x) { return (__float_as_int(x) & 0x7f800000) != 0x7f800000; }
__device__ __forceinline__ float opt_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One workgroup's share of the init: state words [0, 16 + 2 n) <- 0, p <- sigmoid(theta).  `item` selects the slice
// [item count, (item + 1) count) of every segment (count = a.count[s], the per-item count) and `state` is that item's block; the
// single-song kernel is item 0 of one.
__device__ __forceinline__ void opt_init(const OptArgs& a, int item, int32_t* __restrict__ state) {
    const int tid = threadIdx.x;
    const int words = kOptHdr + 2 * a.n_params;
    for (int w = tid; w < words; w += kOptWG) state[w] = 0;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        const int64_t off = (int64_t)item * a.count[s];
        const float* __restrict__ th = a.theta[s] + off;
        float* __restrict__ p = a.p[s] + off;
        for (int i = tid; i < a.count[s]; i += kOptWG) p[i] = opt_sigmoid(th[i]);
    }
}
// The sum of the sections' gradient rows at coordinate i, ((g_0 + g_1) + g_2) + ... in fp32 in section order; `bad` collects an
// addend or a partial sum that is not finite (two finite addends may overflow).  One row: the element itself, no addition.
__device__ __forceinline__ float opt_section_sum(const float* __restrict__ dp, int i, int n, int sections, bool& bad) {
    float sum = dp[i];
    bad |= !opt_finite(sum);
    for (int r = 1; r < sections; ++r) {
        const float g = dp[(int64_t)r * n + i];
        bad |= !opt_finite(g);
        sum = sum + g;
        bad |= !opt_finite(sum);
    }
    return sum;
}
// Linked rows: the gradient of the logit that the group led by row l shares at column c, ((g_m0 + g_m1) + ...) in fp32
// over the members m in ascending order, the leader first.  g_m is the member's own chain through the sigmoid, its d_m the section sum
// over ITS rows and p_m read from its own row 0, negated for a follower at the mirrored column (its logit is minus the leader's).
// `bad` collects an addend or a partial sum that is not finite.  A row that leads itself alone: today's g, no addition.
__device__ __forceinline__ float opt_group_sum(const float* __restrict__ dp, const float* __restrict__ p, int l, int c, int n, int sections,
                                               const mst_logit_adam_links& k, const uint8_t* __restrict__ leader, bool& bad) {
    float sum = 0.0f;
    for (int m = l; m < k.rows; ++m) {
        if (leader[m] != l) continue;
        const int j = m * k.cols + c;
        const float pm = p[j];
        const float d = opt_section_sum(dp, j, n, sections, bad);
        float g = (d * (1.0f - pm)) * pm;
        if (m != l && c == k.mirror_col) g = -g;
        bad |= !opt_finite(g);
        if (m == l) {
            sum = g;
        } else {
            sum = sum + g;
            bad |= !opt_finite(sum);
        }
    }
    return sum;
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_init(OptArgs a, int32_t* __restrict__ state) { opt_init(a, 0, state); }
// ... for one parameter set whose p has `sections` equal rows: the init of the single kernel, its p written to every row
__global__ __launch_bounds__(kOptWG) void k_logit_adam_init_sections(OptArgs a, int32_t* __restrict__ state, int sections) {
    const int tid = threadIdx.x;
    const int words = kOptHdr + 2 * a.n_params;
    for (int w = tid; w < words; w += kOptWG) state[w] = 0;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        const float* __restrict__ th = a.theta[s];
        float* __restrict__ p = a.p[s];
        const int n = a.count[s];
        for (int i = tid; i < n; i += kOptWG) {
            const float pi = opt_sigmoid(th[i]);
            for (int r = 0; r < sections; ++r) p[(int64_t)r * n + i] = pi;
        }
    }
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_init_batch(OptArgs a, int32_t* __restrict__ state) {
    const int item = blockIdx.x;
    opt_init(a, item, state + (int64_t)item * (kOptHdr + 2 * a.n_params));
}
// ... for `items` parameter sets with `sections` equal rows of p each: workgroup b is the sections init on item b - its slice of
// theta, its state block, rows [b sections, (b + 1) sections) of p
__global__ __launch_bounds__(kOptWG) void k_logit_adam_init_sections_batch(OptArgs a, int32_t* __restrict__ state, int sections) {
    const int tid = threadIdx.x;
    const int item = blockIdx.x;
    const int words = kOptHdr + 2 * a.n_params;
    state += (int64_t)item * words;
    for (int w = tid; w < words; w += kOptWG) state[w] = 0;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        const int n = a.count[s];
        const float* __restrict__ th = a.theta[s] + (int64_t)item * n;
        float* __restrict__ p = a.p[s] + (int64_t)item * sections * n;
        for (int i = tid; i < n; i += kOptWG) {
            const float pi = opt_sigmoid(th[i]);
            for (int r = 0; r < sections; ++r) p[(int64_t)r * n + i] = pi;
        }
    }
}
// ... with linked rows in segment `links.segment`: a follower row takes its leader's logits, minus them at the mirrored
// column, before the sigmoid; the lane of a follower coordinate reads the leader's logit, which no lane writes
__global__ __launch_bounds__(kOptWG) void k_logit_adam_init_linked(OptArgs a, int32_t* __restrict__ state, int sections,
                                                                   mst_logit_adam_links links) {
    const int tid = threadIdx.x;
    const int item = blockIdx.x;
    const int words = kOptHdr + 2 * a.n_params;
    state += (int64_t)item * words;
    for (int w = tid; w < words; w += kOptWG) state[w] = 0;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        const int n = a.count[s];
        float* th = a.theta[s] + (int64_t)item * n;
        float* __restrict__ p = a.p[s] + (int64_t)item * sections * n;
        for (int i = tid; i < n; i += kOptWG) {
            float ti = th[i];
            if (s == links.segment) {
                const int row = i / links.cols, c = i - row * links.cols;
                const int l = links.leader[row];
                if (l != row) {
                    ti = th[l * links.cols + c];
                    if (c == links.mirror_col) ti = -ti;
                    th[i] = ti;
                }
            }
            const float pi = opt_sigmoid(ti);
            for (int r = 0; r < sections; ++r) p[(int64_t)r * n + i] = pi;
        }
    }
}

// One workgroup's whole step over its item's slices: the body of the four kernels below.  term(k) is loss term k of this item, `row`
// its history row, `state` its block (header, first moments, second moments).  kBest adds the best-iterate bookkeeping on `best`;
// the arithmetic of the update is the same statements either way.
// kSections (mst_logit_adam_step_sections): grad_p and p have `sections` rows of `count`, `count` elements apart; the gradient of a
// coordinate is the sum of its rows (opt_section_sum) and the new p goes to every row.  Everything else is the same statements.
// With kSections an item's rows of p and grad_p begin item * sections * count in (mst_logit_adam_step_sections_batch); the single
// kernels run it with item = 0, where that is no offset at all.
// kLinked (mst_logit_adam_step_linked; with kSections): in segment links->segment the rows of a group share one logit per
// column.  Only the lane of a leader coordinate acts: the gradient is opt_group_sum over the members, the Adam statements run on the
// leader's moments and logit, and theta, p and the snapshot are written for every member (minus the logit at the mirrored column of a
// follower).  Lanes of follower coordinates write nothing, so their moment words stay zero.  `leader` is the map in LDS, written by
// the kernel before the call; the first barrier below publishes it.  The other instantiations have none of this code.
template <bool kBest, class Term, bool kSections = false, bool kLinked = false>
__device__ __forceinline__ void opt_step(const OptArgs& a, int item, Term term, float* __restrict__ row, double lr, double beta1,
                                         double beta2, float eps, int32_t* __restrict__ state, OptBest best = OptBest{},
                                         int sections = 1, const mst_logit_adam_links* links = nullptr,
                                         const uint8_t* __restrict__ leader = nullptr) {
    __shared__ int s_bad;
    __shared__ int s_best;
    __shared__ float s_step, s_c2;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_bad = 0;
        if (kBest) {  // the verdict on this iteration's loss, for every lane after the barrier below; it holds only if the step is taken
            int verdict = best.block[3] ? kBestSettled : 0;
            float sum = 0.0f;  // the sum lane 0 writes to row[0] below: the same additions in the same order
            for (int k = 0; k < a.n_terms; ++k) sum += term(k);
            if (!best.block[0] || sum < __int_as_float(best.block[1]) - best.min_delta) verdict |= kBestImproved;
            s_best = verdict;
        }
    }
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        if (!a.grad_p[s]) continue;
        // an item's rows of grad_p (and of p below) lie item * sections * count in; its theta item * count
        const float* __restrict__ dp = a.grad_p[s] + (kSections ? (int64_t)item * sections * a.count[s] : (int64_t)item * a.count[s]);
        if constexpr (kLinked) {
            if (s == links->segment) {  // every row is a member of one group: its leader's lane looks at it
                const float* __restrict__ p = a.p[s] + (int64_t)item * sections * a.count[s];
                for (int i = tid; i < a.count[s]; i += kOptWG) {
                    const int l = i / links->cols;
                    if (leader[l] == l) opt_group_sum(dp, p, l, i - l * links->cols, a.count[s], sections, *links, leader, bad);
                }
                continue;
            }
        }
        if (kSections) {
            for (int i = tid; i < a.count[s]; i += kOptWG) opt_section_sum(dp, i, a.count[s], sections, bad);
        } else {
            for (int i = tid; i < a.count[s]; i += kOptWG) bad |= !opt_finite(dp[i]);
        }
    }
    if (tid < a.n_terms) bad |= !opt_finite(term(tid));
    if (bad) atomicMax(&s_bad, 1);
    if (tid == 0) {  // the two bias corrections of step t = state[0] + 1, in float64, rounded once
        const double t = (double)(state[0] + 1);
        s_step = (float)(-(lr / (1.0 - pow(beta1, t))));
        s_c2 = (float)sqrt(1.0 - pow(beta2, t));
    }
    __syncthreads();
    const bool settled = kBest && (s_best & kBestSettled);
    const bool stop = s_bad != 0;
    const bool improved = kBest && !stop && (s_best & kBestImproved);  // and not settled: a settled item returns before it is used
    if (tid == 0) {
        float sum = 0.0f;  // the script's `loss = 0; loss += value`, left to right
        for (int k = 0; k < a.n_terms; ++k) {
            const float value = term(k);
            sum += value;
            row[1 + k] = value;
        }
        row[0] = sum;
        const int32_t iteration = state[3];
        if (settled) {  // frozen: the row and the call count, nothing else - not even the status of a non-finite input
            state[3] = iteration + 1;
        } else {
            if (stop && !state[1]) {
                state[1] = MST_OPT_STATUS_NONFINITE;
                state[2] = iteration;
            }
            state[3] = iteration + 1;
            if (!stop) state[0] += 1;
            if (kBest && !stop) {  // a non-finite iteration leaves the best block alone, the wait count too
                int32_t wait = 0;
                if (improved) {
                    float* __restrict__ best_row = reinterpret_cast<float*>(best.block + kBestHdr + a.n_params);
                    best_row[0] = sum;
                    for (int k = 0; k < a.n_terms; ++k) best_row[1 + k] = term(k);
                    best.block[0] = iteration + 1;
                    best.block[1] = __float_as_int(sum);
                } else {
                    wait = best.block[2] + 1;
                }
                best.block[2] = wait;
                if (best.patience > 0 && wait >= best.patience) best.block[3] = iteration + 1;  // frozen from the next call on
            }
        }
    }
    if (settled || stop) return;
    float* __restrict__ snap = kBest ? reinterpret_cast<float*>(best.block + kBestHdr) : nullptr;
    const float step = s_step, c2 = s_c2, b2 = (float)beta2, w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2);
    float* __restrict__ m_all = reinterpret_cast<float*>(state + kOptHdr);
    float* __restrict__ v_all = m_all + a.n_params;
    int at = 0;
#pragma unroll
    for (int s = 0; s < MST_OPT_MAX_SEGMENTS; ++s) {
        if (s >= a.n_segments) break;
        const int n = a.count[s];
        if (a.grad_p[s]) {  // a NULL gradient is a parameter without .grad: torch skips it, its logits, moments and p keep their bits
            const int64_t off = (int64_t)item * n;
            const int64_t rows = kSections ? off * sections : off;  // where this item's rows of p and grad_p begin
            const float* __restrict__ dp = a.grad_p[s] + rows;
            float* __restrict__ th = a.theta[s] + off;
            float* __restrict__ p = a.p[s] + rows;
            float* __restrict__ m = m_all + at;
            float* __restrict__ v = v_all + at;
            if constexpr (kLinked) {
                if (s == links->segment) {
                    const int cols = links->cols;
                    for (int i = tid; i < n; i += kOptWG) {
                        const int l = i / cols, c = i - l * cols;
                        if (leader[l] != l) continue;
                        bool ignored = false;
                        const float g = opt_group_sum(dp, p, l, c, n, sections, *links, leader, ignored);
                        const float mi = m[i] + w1 * (g - m[i]);
                        const float vi = v[i] * b2 + (w2 * g) * g;
                        const float ti = th[i] + (step * mi) / (sqrtf(vi) / c2 + eps);
                        m[i] = mi;
                        v[i] = vi;
                        for (int f = l; f < links->rows; ++f) {  // the members, the leader first: this lane alone touches them
                            if (leader[f] != l) continue;
                            const int j = f * cols + c;
                            if (improved) snap[at + j] = th[j];  // the member's own logit the loss was evaluated at
                            const float tj = (f != l && c == links->mirror_col) ? -ti : ti;
                            th[j] = tj;
                            const float pn = opt_sigmoid(tj);
                            for (int r = 0; r < sections; ++r) p[(int64_t)r * n + j] = pn;
                        }
                    }
                    at += n;
                    continue;
                }
            }
            for (int i = tid; i < n; i += kOptWG) {
                const float pi = p[i];  // with sections: row 0, every row holds the same bits
                bool ignored = false;
                const float dpi = kSections ? opt_section_sum(dp, i, n, sections, ignored) : dp[i];
                const float g = (dpi * (1.0f - pi)) * pi;
                const float mi = m[i] + w1 * (g - m[i]);
                const float vi = v[i] * b2 + (w2 * g) * g;
                if (improved) snap[at + i] = th[i];  // the logit the loss was evaluated at; this lane is the only one that touches i
                const float ti = th[i] + (step * mi) / (sqrtf(vi) / c2 + eps);
                m[i] = mi;
                v[i] = vi;
                th[i] = ti;
                const float pn = opt_sigmoid(ti);
                p[i] = pn;
                if (kSections)
                    for (int r = 1; r < sections; ++r) p[(int64_t)r * n + i] = pn;
            }
        } else if (improved) {
            const float* __restrict__ th = a.theta[s] + (int64_t)item * n;
            for (int i = tid; i < n; i += kOptWG) snap[at + i] = th[i];
        }
        at += n;
    }
}

__global__ __launch_bounds__(kOptWG) void k_logit_adam_step(OptArgs a, float* __restrict__ row, double lr, double beta1, double beta2,
                                                            float eps, int32_t* __restrict__ state) {
    opt_step<false>(a, 0, [&](int k) { return *a.term[k]; }, row, lr, beta1, beta2, eps, state);
}
// Batched fits (include/diffmst_hip.h): workgroup b is the single kernel on item b - its slice of every segment, row b of the dense
// (items, n_terms) loss terms, history row b, state block b, its own "not finite" flag in its own LDS.  Workgroups exchange nothing.
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_batch(OptArgs a, const float* __restrict__ terms, float* __restrict__ rows,
                                                                  double lr, double beta1, double beta2, float eps,
                                                                  int32_t* __restrict__ state) {
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    opt_step<false>(a, item, [&](int k) { return mine[k]; }, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                    state + (int64_t)item * (kOptHdr + 2 * a.n_params));
}
// The same two with the best-iterate block (include/diffmst_hip.h): `best.block` is the first item's, item b's lies
// b (16 + n_params + 1 + MST_OPT_MAX_TERMS) words further.
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_best(OptArgs a, float* __restrict__ row, double lr, double beta1,
                                                                 double beta2, float eps, int32_t* __restrict__ state, OptBest best) {
    opt_step<true>(a, 0, [&](int k) { return *a.term[k]; }, row, lr, beta1, beta2, eps, state, best);
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_best_batch(OptArgs a, const float* __restrict__ terms,
                                                                       float* __restrict__ rows, double lr, double beta1, double beta2,
                                                                       float eps, int32_t* __restrict__ state, OptBest best) {
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    best.block += (int64_t)item * (kBestHdr + a.n_params + 1 + MST_OPT_MAX_TERMS);
    opt_step<true>(a, item, [&](int k) { return mine[k]; }, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                   state + (int64_t)item * (kOptHdr + 2 * a.n_params), best);
}

// One parameter set, `sections` gradient rows (include/diffmst_hip.h): the single kernels' body on the summed gradient.
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_sections(OptArgs a, float* __restrict__ row, double lr, double beta1,
                                                                     double beta2, float eps, int32_t* __restrict__ state, int sections) {
    auto term = [&](int k) { return *a.term[k]; };
    opt_step<false, decltype(term), true>(a, 0, term, row, lr, beta1, beta2, eps, state, OptBest{}, sections);
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_best_sections(OptArgs a, float* __restrict__ row, double lr, double beta1,
                                                                          double beta2, float eps, int32_t* __restrict__ state,
                                                                          OptBest best, int sections) {
    auto term = [&](int k) { return *a.term[k]; };
    opt_step<true, decltype(term), true>(a, 0, term, row, lr, beta1, beta2, eps, state, best, sections);
}
// `items` parameter sets with `sections` gradient rows each (include/diffmst_hip.h): workgroup b is the sections kernel on item b,
// with the batch kernels' row b of the dense loss terms, history row b, state block b and best block b.  Workgroups exchange nothing.
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_sections_batch(OptArgs a, const float* __restrict__ terms,
                                                                           float* __restrict__ rows, double lr, double beta1,
                                                                           double beta2, float eps, int32_t* __restrict__ state,
                                                                           int sections) {
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    auto term = [&](int k) { return mine[k]; };
    opt_step<false, decltype(term), true>(a, item, term, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                                          state + (int64_t)item * (kOptHdr + 2 * a.n_params), OptBest{}, sections);
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_best_sections_batch(OptArgs a, const float* __restrict__ terms,
                                                                                float* __restrict__ rows, double lr, double beta1,
                                                                                double beta2, float eps, int32_t* __restrict__ state,
                                                                                OptBest best, int sections) {
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    best.block += (int64_t)item * (kBestHdr + a.n_params + 1 + MST_OPT_MAX_TERMS);
    auto term = [&](int k) { return mine[k]; };
    opt_step<true, decltype(term), true>(a, item, term, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                                         state + (int64_t)item * (kOptHdr + 2 * a.n_params), best, sections);
}
// The two kernels above with linked rows (include/diffmst_hip.h).  The map is a kernel argument of its own, after every
// argument of the kernels above; lane r copies leader[r] to LDS (MST_OPT_MAX_LINK_ROWS == the workgroup size) and the step's first
// barrier publishes it.
static_assert(MST_OPT_MAX_LINK_ROWS == kOptWG, "one lane per entry of the leader map");
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_linked(OptArgs a, const float* __restrict__ terms, float* __restrict__ rows,
                                                                   double lr, double beta1, double beta2, float eps,
                                                                   int32_t* __restrict__ state, int sections, mst_logit_adam_links links) {
    __shared__ uint8_t s_leader[MST_OPT_MAX_LINK_ROWS];
    s_leader[threadIdx.x] = links.leader[threadIdx.x];
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    auto term = [&](int k) { return mine[k]; };
    opt_step<false, decltype(term), true, true>(a, item, term, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                                                state + (int64_t)item * (kOptHdr + 2 * a.n_params), OptBest{}, sections, &links, s_leader);
}
__global__ __launch_bounds__(kOptWG) void k_logit_adam_step_best_linked(OptArgs a, const float* __restrict__ terms,
                                                                        float* __restrict__ rows, double lr, double beta1, double beta2,
                                                                        float eps, int32_t* __restrict__ state, OptBest best, int sections,
                                                                        mst_logit_adam_links links) {
    __shared__ uint8_t s_leader[MST_OPT_MAX_LINK_ROWS];
    s_leader[threadIdx.x] = links.leader[threadIdx.x];
    const int item = blockIdx.x;
    const float* __restrict__ mine = terms + (int64_t)item * a.n_terms;
    best.block += (int64_t)item * (kBestHdr + a.n_params + 1 + MST_OPT_MAX_TERMS);
    auto term = [&](int k) { return mine[k]; };
    opt_step<true, decltype(term), true, true>(a, item, term, rows + (int64_t)item * (1 + a.n_terms), lr, beta1, beta2, eps,
                                               state + (int64_t)item * (kOptHdr + 2 * a.n_params), best, sections, &links, s_leader);
}

namespace {
// the segment table as kernel arguments; false for what the kernels do not support
// (a.count and a.n_params are per item: every count must divide by `items`, 1 for the single-song calls)
bool opt_args(const mst_logit_adam_segment* segments, int32_t n_segments, OptArgs& a, int32_t items = 1) {
    if (!segments || n_segments < 1 || n_segments > MST_OPT_MAX_SEGMENTS || items < 1 || items > kOptMaxItems) return false;
    a = OptArgs{};
    int64_t total = 0;
    for (int s = 0; s < n_segments; ++s) {
        const mst_logit_adam_segment& g = segments[s];
        if (!g.theta || !g.p || g.count < 1 || g.count % items || g.count / items > kOptMaxParams || ((uintptr_t)g.theta & 3) ||
            ((uintptr_t)g.p & 3) || ((uintptr_t)g.grad_p & 3))
            return false;
        a.theta[s] = g.theta;
        a.p[s] = g.p;
        a.grad_p[s] = g.grad_p;
        a.count[s] = (int32_t)(g.count / items);
        total += g.count / items;
    }
    if (total > kOptMaxParams) return false;
    a.n_segments = n_segments;
    a.n_params = (int32_t)total;
    return true;
}
// the extra arguments of the `_best` launchers; false for what they refuse
bool opt_best(void* best, double min_delta, int32_t patience, OptBest& b) {
    if (!best || ((uintptr_t)best & 3) || !(min_delta >= 0.0) || !isfinite(min_delta) || !isfinite((float)min_delta) || patience < 0)
        return false;
    b = OptBest{(int32_t*)best, (float)min_delta, patience};
    return true;
}
// the link description of the `_linked` launchers against the segment table; false for what they refuse
bool opt_links(const mst_logit_adam_links* links, const OptArgs& a) {
    if (!links || links->segment < 0 || links->segment >= a.n_segments || links->rows < 1 || links->rows > MST_OPT_MAX_LINK_ROWS ||
        links->cols < 1 || (int64_t)links->rows * links->cols != a.count[links->segment] || links->mirror_col < -1 ||
        links->mirror_col >= links->cols)
        return false;
    for (int r = 0; r < links->rows; ++r) {
        const int l = links->leader[r];
        if (l > r || links->leader[l] != l) return false;
    }
    return true;
}
}  // namespace
}  // namespace mst

using namespace mst;

extern "C" size_t mst_logit_adam_state_bytes(int64_t n_params) {
    if (n_params < 1 || n_params > kOptMaxParams) return 0;
    return ((size_t)kOptHdr + 2 * (size_t)n_params) * 4;
}
extern "C" int mst_logit_adam_init(const mst_logit_adam_segment* segments, int32_t n_segments, void* state, void* stream) {
    OptArgs a;
    if (!opt_args(segments, n_segments, a) || !state || ((uintptr_t)state & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_logit_adam_init, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, (int32_t*)state);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step(const mst_logit_adam_segment* segments, int32_t n_segments, const float* const* loss_terms,
                                   int32_t n_terms, float* history_row, double lr, double beta1, double beta2, double eps, void* state,
                                   void* stream) {
    OptArgs a;
    if (!opt_args(segments, n_segments, a) || !state || ((uintptr_t)state & 3) || !history_row || ((uintptr_t)history_row & 3) ||
        !loss_terms || n_terms < 1 || n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!(lr > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return hipErrorInvalidValue;
    for (int k = 0; k < n_terms; ++k) {
        if (!loss_terms[k] || ((uintptr_t)loss_terms[k] & 3)) return hipErrorInvalidValue;
        a.term[k] = loss_terms[k];
    }
    a.n_terms = n_terms;
    hipLaunchKernelGGL(k_logit_adam_step, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, history_row, lr, beta1, beta2, (float)eps,
                       (int32_t*)state);
    return (int)hipGetLastError();
}

// ---- batched fits: `items` independent optimisations in one launch, one workgroup each ---------------------------------------------
static bool opt_hyper_ok(double lr, double beta1, double beta2, double eps) {
    return lr > 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0;
}
extern "C" size_t mst_logit_adam_batch_state_bytes(int32_t items, int64_t params_per_item) {
    if (items < 1 || items > kOptMaxItems || params_per_item < 1 || params_per_item > kOptMaxParams) return 0;
    return (size_t)items * ((size_t)kOptHdr + 2 * (size_t)params_per_item) * 4;
}
extern "C" int mst_logit_adam_init_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, void* state,
                                         void* stream) {
    OptArgs a;
    if (!opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_logit_adam_init_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, (int32_t*)state);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items,
                                         const float* loss_terms, int32_t n_terms, float* history_rows, double lr, double beta1,
                                         double beta2, double eps, void* state, void* stream) {
    OptArgs a;
    if (!opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3) || !history_rows ||
        ((uintptr_t)history_rows & 3) || !loss_terms || ((uintptr_t)loss_terms & 3) || n_terms < 1 || n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps)) return hipErrorInvalidValue;
    a.n_terms = n_terms;
    hipLaunchKernelGGL(k_logit_adam_step_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms, history_rows, lr,
                       beta1, beta2, (float)eps, (int32_t*)state);
    return (int)hipGetLastError();
}

// ---- the same steps, remembering the best iterate and freezing an item that has stopped improving ---------------------------------
extern "C" size_t mst_logit_adam_best_bytes(int32_t items, int64_t params_per_item) {
    if (items < 1 || items > kOptMaxItems || params_per_item < 1 || params_per_item > kOptMaxParams) return 0;
    return (size_t)items * ((size_t)kBestHdr + (size_t)params_per_item + 1 + MST_OPT_MAX_TERMS) * 4;
}
extern "C" int mst_logit_adam_step_best(const mst_logit_adam_segment* segments, int32_t n_segments, const float* const* loss_terms,
                                        int32_t n_terms, float* history_row, double lr, double beta1, double beta2, double eps,
                                        double min_delta, int32_t patience, void* state, void* best, void* stream) {
    OptArgs a;
    OptBest b;
    if (!opt_args(segments, n_segments, a) || !state || ((uintptr_t)state & 3) || !history_row || ((uintptr_t)history_row & 3) ||
        !loss_terms || n_terms < 1 || n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps) || !opt_best(best, min_delta, patience, b)) return hipErrorInvalidValue;
    for (int k = 0; k < n_terms; ++k) {
        if (!loss_terms[k] || ((uintptr_t)loss_terms[k] & 3)) return hipErrorInvalidValue;
        a.term[k] = loss_terms[k];
    }
    a.n_terms = n_terms;
    hipLaunchKernelGGL(k_logit_adam_step_best, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, history_row, lr, beta1, beta2,
                       (float)eps, (int32_t*)state, b);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step_best_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items,
                                              const float* loss_terms, int32_t n_terms, float* history_rows, double lr, double beta1,
                                              double beta2, double eps, double min_delta, int32_t patience, void* state, void* best,
                                              void* stream) {
    OptArgs a;
    OptBest b;
    if (!opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3) || !history_rows ||
        ((uintptr_t)history_rows & 3) || !loss_terms || ((uintptr_t)loss_terms & 3) || n_terms < 1 || n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps) || !opt_best(best, min_delta, patience, b)) return hipErrorInvalidValue;
    a.n_terms = n_terms;
    hipLaunchKernelGGL(k_logit_adam_step_best_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms, history_rows, lr,
                       beta1, beta2, (float)eps, (int32_t*)state, b);
    return (int)hipGetLastError();
}

// ---- one parameter set, several gradient rows: the sections of a song fitted together ----------------------------------------------
constexpr int kOptMaxSections = MST_OPT_MAX_SECTIONS;
extern "C" int mst_logit_adam_init_sections(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t sections, void* state,
                                            void* stream) {
    OptArgs a;
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a) || !state || ((uintptr_t)state & 3))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_logit_adam_init_sections, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, (int32_t*)state, (int)sections);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step_sections(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t sections,
                                            const float* const* loss_terms, int32_t n_terms, float* history_row, double lr, double beta1,
                                            double beta2, double eps, double min_delta, int32_t patience, void* state, void* best,
                                            void* stream) {
    OptArgs a;
    OptBest b{};
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a) || !state || ((uintptr_t)state & 3) ||
        !history_row || ((uintptr_t)history_row & 3) || !loss_terms || n_terms < 1 || n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps) || (best && !opt_best(best, min_delta, patience, b))) return hipErrorInvalidValue;
    for (int k = 0; k < n_terms; ++k) {
        if (!loss_terms[k] || ((uintptr_t)loss_terms[k] & 3)) return hipErrorInvalidValue;
        a.term[k] = loss_terms[k];
    }
    a.n_terms = n_terms;
    if (best)
        hipLaunchKernelGGL(k_logit_adam_step_best_sections, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, history_row, lr, beta1,
                           beta2, (float)eps, (int32_t*)state, b, (int)sections);
    else
        hipLaunchKernelGGL(k_logit_adam_step_sections, dim3(1), dim3(kOptWG), 0, (hipStream_t)stream, a, history_row, lr, beta1, beta2,
                           (float)eps, (int32_t*)state, (int)sections);
    return (int)hipGetLastError();
}

// ---- several parameter sets, several gradient rows each: a batch of sectioned fits ------------------------------------------------
extern "C" int mst_logit_adam_init_sections_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items,
                                                  int32_t sections, void* state, void* stream) {
    OptArgs a;
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_logit_adam_init_sections_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, (int32_t*)state,
                       (int)sections);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step_sections_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items,
                                                  int32_t sections, const float* loss_terms, int32_t n_terms, float* history_rows,
                                                  double lr, double beta1, double beta2, double eps, double min_delta, int32_t patience,
                                                  void* state, void* best, void* stream) {
    OptArgs a;
    OptBest b{};
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3) ||
        !history_rows || ((uintptr_t)history_rows & 3) || !loss_terms || ((uintptr_t)loss_terms & 3) || n_terms < 1 ||
        n_terms > MST_OPT_MAX_TERMS)
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps) || (best && !opt_best(best, min_delta, patience, b))) return hipErrorInvalidValue;
    a.n_terms = n_terms;
    if (best)
        hipLaunchKernelGGL(k_logit_adam_step_best_sections_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms,
                           history_rows, lr, beta1, beta2, (float)eps, (int32_t*)state, b, (int)sections);
    else
        hipLaunchKernelGGL(k_logit_adam_step_sections_batch, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms,
                           history_rows, lr, beta1, beta2, (float)eps, (int32_t*)state, (int)sections);
    return (int)hipGetLastError();
}

// ---- the same, with rows of one segment linked: tied logits and a mirrored column (stereo pairs) -----------------------------------
extern "C" int mst_logit_adam_init_linked(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                                          const mst_logit_adam_links* links, void* state, void* stream) {
    OptArgs a;
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3) ||
        !opt_links(links, a))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_logit_adam_init_linked, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, (int32_t*)state, (int)sections,
                       *links);
    return (int)hipGetLastError();
}
extern "C" int mst_logit_adam_step_linked(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                                          const mst_logit_adam_links* links, const float* loss_terms, int32_t n_terms,
                                          float* history_rows, double lr, double beta1, double beta2, double eps, double min_delta,
                                          int32_t patience, void* state, void* best, void* stream) {
    OptArgs a;
    OptBest b{};
    if (sections < 1 || sections > kOptMaxSections || !opt_args(segments, n_segments, a, items) || !state || ((uintptr_t)state & 3) ||
        !history_rows || ((uintptr_t)history_rows & 3) || !loss_terms || ((uintptr_t)loss_terms & 3) || n_terms < 1 ||
        n_terms > MST_OPT_MAX_TERMS || !opt_links(links, a))
        return hipErrorInvalidValue;
    if (!opt_hyper_ok(lr, beta1, beta2, eps) || (best && !opt_best(best, min_delta, patience, b))) return hipErrorInvalidValue;
    a.n_terms = n_terms;
    if (best)
        hipLaunchKernelGGL(k_logit_adam_step_best_linked, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms, history_rows,
                           lr, beta1, beta2, (float)eps, (int32_t*)state, b, (int)sections, *links);
    else
        hipLaunchKernelGGL(k_logit_adam_step_linked, dim3(items), dim3(kOptWG), 0, (hipStream_t)stream, a, loss_terms, history_rows, lr,
                           beta1, beta2, (float)eps, (int32_t*)state, (int)sections, *links);
    return (int)hipGetLastError();
}
