/* diffmst_hip.h - C ABI of the MI355X-native Diff-MST mix-console hot path.
 *
 * The reference (sai-soum/Diff-MST) is pure Python and has no FFI; its seam for this
 * path is the operator ring of six functions imported from dasp_pytorch.functional
 * (reference mst/modules.py:7-14, called at :231-312) plus the loss objects called as
 * loss(pred, target) (reference mst/system.py:331-338).  This header is the C-ABI
 * ring a maintainer binds instead (ctypes stub: INTEGRATION.md): stateless launchers
 * over caller-owned device buffers.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless stated; the caller (PyTorch's caching
 *    allocator) owns all memory; nothing is allocated, freed or retained here;
 *  - all signals are fp32; tracks are (bs, n_tracks, n_samples) with unit sample stride
 *    and `track_row_stride` elements between consecutive (b,t) rows (reference
 *    mst/system.py:258 passes a last-dim slice - SURVEY App. C.7); stereo signals are
 *    dense (bs, 2, n_samples);
 *  - every launcher enqueues on `stream` and returns immediately; return value is a
 *    hipError_t-compatible int (0 = ok), never an exception / abort;
 *  - semantic errors keep the reference's Python exceptions: the launcher only writes
 *    a code to `status` (see mst_console_forward) and the host wrapper raises;
 *  - re-entrant: the library keeps NO process-wide mutable state (no stream pools, no caches, no environment
 *    switches in the default build); everything a call needs arrives through its arguments.
 */
#ifndef DIFFMST_HIP_H
#define DIFFMST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MST_NUM_TRACK_PARAMS 27  /* reference mst/modules.py:182 */
#define MST_NUM_FX_PARAMS 25     /* :183 */
#define MST_NUM_MASTER_PARAMS 26 /* :184 */

/* flag bits = keyword flags of AdvancedMixConsole.forward (reference mst/modules.py:316-329) */
#define MST_USE_TRACK_INPUT_FADER 0x01u
#define MST_USE_TRACK_EQ 0x02u
#define MST_USE_TRACK_COMPRESSOR 0x04u
#define MST_USE_TRACK_PANNER 0x08u
#define MST_USE_FX_BUS 0x10u /* stereo send bus + noise-shaped reverberation (reference mst/modules.py:275-284); needs mst_console_fx */
#define MST_USE_MASTER_BUS 0x20u
#define MST_USE_OUTPUT_FADER 0x40u
#define MST_SAVE_FOR_BACKWARD 0x100u /* keep intermediates in the workspace for mst_console_backward */
#define MST_NO_RANGE_CHECK 0x400u   /* the parameter tensors hold DENORMALISED values (forward_mix_console, reference
                                       mst/modules.py:186-314, which applies whatever it is given): no range check; the
                                       caller passes lo = 0, hi = 1 so that the map v*(hi-lo)+lo is the identity and the
                                       returned gradients are w.r.t. the denormalised values */
#define MST_BWD_PREPARED 0x800u     /* mst_console_backward only: mst_console_backward_prepare has already run on this workspace */
#define MST_SPLIT_BATCH 0x1000u     /* ABI v9, mst_console_forward_overlapped / _backward_overlapped: run the call as two halves of the
                                       batch on two streams (see mst_console_overlap); must be set - or not - in BOTH calls over a
                                       workspace, it selects the workspace layout.  Ignored (both calls alike) when bs < 2, with
                                       MST_USE_FX_BUS and on the gain + pan fast path */
#define MST_DEV_MULTIPASS_EQ 0x200u /* developer/test switch: keep the EQ carry scan in its own kernel (zero-state pass,
                                       carry scan, run) even when a row is short enough (<= 262144 samples) for the
                                       in-wave scans of the two-kernel path; longer rows always take three kernels */

/* *status after mst_console_forward: 0 = all parameters in [0,1]; otherwise 1000 - code with
 * code = 1 + k           track parameter index k out of range   (reference mst/modules.py:353-392)
 *        1 + 27 + k      fx-bus parameter index k out of range  (:394-422)
 *        1 + 52 + k      master-bus parameter index k           (:424-460)
 * the smallest code wins (atomic max of 1000-code), which is the reference's dictionary
 * iteration order (:79-97).  *status is only ever raised (atomic max): the caller zeroes it once and may let
 * several calls accumulate into it before reading (deferred validation).
 *
 * MST_STATUS_EXCHANGE_TIMEOUT (2000, above every range code): a kernel of the call gave up waiting for a value that another
 * workgroup of the SAME launch publishes (the block / tile aggregates of the recurrences are exchanged inside the run launches
 * instead of by a launch of their own).  The outputs of that call are poisoned (NaN) and must not be used; the Python binding
 * raises RuntimeError at its next status read (validate="sync": right after the forward; "deferred": check_parameters()).
 * Forward progress of those waits rests on ONE assumption about the hardware, which HIP does not promise: the workgroups of a launch
 * are dispatched in ascending order of their linear id (observed on gfx950, MI355X_MICROARCH.md) - a waiting workgroup only ever waits
 * for workgroups with lower ids, which are therefore resident or finished.  Every wait is bounded (MST_GRAN_SPINS polls), so a
 * platform that breaks the assumption produces this status, not a hang. */
#define MST_STATUS_EXCHANGE_TIMEOUT 2000

typedef struct mst_console_desc {
    int32_t bs;
    int32_t n_tracks;
    int64_t n_samples;
    int64_t track_row_stride; /* elements between (b,t) rows of `tracks` */
    float sample_rate;
    uint32_t flags;
    int32_t track_lookahead;  /* 2048, reference mst/modules.py:250 */
    int32_t master_lookahead; /* 1024, reference mst/modules.py:304 */
    /* denormalisation ranges v*(hi-lo)+lo, reference mst/modules.py:71-72,121-181 */
    float track_lo[MST_NUM_TRACK_PARAMS], track_hi[MST_NUM_TRACK_PARAMS];
    float master_lo[MST_NUM_MASTER_PARAMS], master_hi[MST_NUM_MASTER_PARAMS];
    /* fx bus (MST_USE_FX_BUS): ranges of the 25 reverberation parameters (band gains, band decays, mix - forward() forces the mix to
     * 1, mst/modules.py:420; under MST_NO_RANGE_CHECK the given value is applied), impulse-response length and band-pass length of
     * dasp_pytorch.functional.noise_shaped_reverberation as the reference calls it (:277-283: 65536, 1023) */
    float fx_lo[MST_NUM_FX_PARAMS], fx_hi[MST_NUM_FX_PARAMS];
    int32_t fx_ir_samples;     /* multiple of 4096 */
    int32_t fx_bandpass_taps;  /* odd, <= 1023 */
} mst_console_desc;

/* Inputs of the fx bus that are not parameters (all device pointers, caller-owned, read-only):
 *   noise    (bs*2, 12, fx_ir_samples + fx_bandpass_taps - 1) standard-normal samples - the reference draws them inside the op
 *            with torch.randn on every call; the caller draws them here (or passes fixed ones: tests)
 *   filters  (12, fx_bandpass_taps) octave-band FIR filterbank (a constant table built by the host wrapper, like the Bark
 *            filterbank of the AudioFeatureLoss)
 *   tables   mst_console_fx_tables_bytes() bytes filled once by mst_console_fx_init_tables() */
typedef struct mst_console_fx {
    const float* noise;
    const float* filters;
    const void* tables;
} mst_console_fx;
size_t mst_console_fx_tables_bytes(void);
int mst_console_fx_init_tables(void* tables, void* stream);

/* Library / ABI version (bumped when a signature changes). */
int mst_abi_version(void);

/* Bytes of scratch the console needs for `d` (includes everything forward saves for backward). */
size_t mst_console_workspace_bytes(const mst_console_desc* d);

/* AdvancedMixConsole.forward_mix_console (reference mst/modules.py:186-314) incl. the
 * denormalise + range check of :79-97: per-track gain -> 6-biquad EQ -> compressor -> pan ->
 * bus sum -> master gain/EQ/stereo-linked compressor -> output fader.
 *   tracks            (bs, n_tracks, n_samples) fp32, see strides above
 *   track_params      (bs, n_tracks, 27) normalised [0,1], dense
 *   fx_bus_params     (bs, 25) - range-checked; used when MST_USE_FX_BUS is set
 *   fx                NULL unless MST_USE_FX_BUS
 *   master_bus_params (bs, 26)
 *   mix               (bs, 2, n_samples) out
 *   mixed_tracks      (bs, 2, n_tracks, n_samples) out, or NULL to skip the API-only copy
 *   status            one int32 on the device, see codes above
 *   workspace         >= mst_console_workspace_bytes(d), 256-byte aligned */
int mst_console_forward(const mst_console_desc* d, const float* tracks, const float* track_params,
                        const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                        float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same call (ABI v8) with the verdict of the range check MIRRORED to the host as soon as it exists: the parameters are checked by
 * the first launch of the forward; right behind it - ahead of every other launch - *status is copied to `status_host` (pinned host
 * memory, one int32) and `status_event` (a hipEvent_t, may be NULL) is recorded.  A caller that wants the reference's immediate
 * ValueError (mst/modules.py:86-89) enqueues the whole forward, then waits for THAT event - 20 us into the call - instead of for the
 * mix: the device never idles behind the host.  Codes raised by later launches of the call (MST_STATUS_EXCHANGE_TIMEOUT) are not in
 * the mirrored value; the device word is sticky and the next mirrored call (or any read of *status) sees them. */
int mst_console_forward_mirrored(const mst_console_desc* d, const float* tracks, const float* track_params,
                                 const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                 float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                 void* stream, int32_t* status_host, void* status_event);

/* ABI v9: the same forward as two HALVES of the batch that overlap on the device (d->flags & MST_SPLIT_BATCH; without the flag this is
 * mst_console_forward).  The mixes of a call are independent (reference mst/modules.py:186-314 has no cross-batch term), so mixes
 * [0, bs / 2) run on `stream` and the rest on `ov->side_stream`, each over its own part of the workspace: the latency-bound stretches of
 * one half (the fp64 design chains of the first launch, the 2 x bs / 2 master-bus rows at one wave per SIMD) run beside the other half's
 * occupancy-full track kernels.  Same kernels and arithmetic per mix: the results are bit-identical to the unsplit call.
 * The library stays stateless: the caller LENDS the side stream and two events (created once, reused by every call, never shared by two
 * calls in flight); the call records `fork_event` on `stream`, makes the side stream wait for it, and before it returns makes `stream`
 * wait for `join_event` recorded behind the side stream's last launch - to the caller everything is ordered on `stream` as before
 * (memory handed to the call may be reused or freed in stream order on `stream`; the pattern is capturable into a hipGraph). */
typedef struct mst_console_overlap {
    void* side_stream; /* hipStream_t, not `stream` */
    void* fork_event;  /* hipEvent_t */
    void* join_event;  /* hipEvent_t */
} mst_console_overlap;
int mst_console_forward_overlapped(const mst_console_desc* d, const float* tracks, const float* track_params,
                                   const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                   float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream, const mst_console_overlap* ov);

/* Reverse-mode of the above (what autograd does through the reference's op graph).
 * `workspace` must be the buffer a forward call with MST_SAVE_FOR_BACKWARD filled, untouched.
 *   grad_mix           (bs, 2, n_samples)
 *   grad_mixed_tracks  (bs, 2, n_tracks, n_samples) or NULL
 *   grad_track_params  (bs, n_tracks, 27) out (w.r.t. the NORMALISED parameters)
 *   grad_master_params (bs, 26) out
 *   grad_fx_params     (bs, 25) out, or NULL (written only when MST_USE_FX_BUS; the "mix" column gets 0 when the call forced it to 1 -
 *                      AdvancedMixConsole.forward, reference mst/modules.py:420 - and the true gradient of
 *                      (1 - mix) fx_in + mix wet under MST_NO_RANGE_CHECK, i.e. forward_mix_console)
 *   grad_tracks        (bs, n_tracks, n_samples) dense out, or NULL when tracks need no grad */
int mst_console_backward(const mst_console_desc* d, const float* tracks, const float* track_params,
                         const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                         const float* grad_mix, const float* grad_mixed_tracks, float* grad_track_params,
                         float* grad_fx_params, float* grad_master_params, float* grad_tracks, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);
/* ... over a workspace that mst_console_forward_overlapped filled with the same d->flags (MST_SPLIT_BATCH included) */
int mst_console_backward_overlapped(const mst_console_desc* d, const float* tracks, const float* track_params,
                                    const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                    const float* grad_mix, const float* grad_mixed_tracks, float* grad_track_params,
                                    float* grad_fx_params, float* grad_master_params, float* grad_tracks, int32_t* status,
                                    void* workspace, size_t workspace_bytes, void* stream, const mst_console_overlap* ov);
/* status (ABI v7; may be null): the forward's status word, raised to MST_STATUS_EXCHANGE_TIMEOUT by a backward launch whose
 * in-launch exchange gave up - the gradients of that call are poisoned. */

/* The part of the backward that depends only on what forward saved (the all-pole carry scan of the coefficient-gradient
 * pass, 15 us at 64 x 262144): a caller may enqueue it on ANOTHER stream once forward has finished there, where it overlaps
 * with whatever runs between the two calls (the loss), make `stream` of mst_console_backward wait for it and pass
 * MST_BWD_PREPARED in d->flags.  Without the flag mst_console_backward runs it itself.  (diffmst_hip/modules.py does this.) */
int mst_console_backward_prepare(const mst_console_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-resolution STFT loss: auraloss.freq.MultiResolutionSTFTLoss as configured by the
 * reference (configs/models/naive.yaml:54-68; called as loss(pred, target), mst/system.py:331).
 * pred / target are (rows, n_samples) dense fp32 with rows = bs * channels. */
#define MST_MAX_RESOLUTIONS 8
typedef struct mst_mrstft_desc {
    int32_t rows;
    int64_t n_samples;
    int32_t n_res;
    int32_t fft_size[MST_MAX_RESOLUTIONS];   /* powers of two, 128..8192 */
    int32_t hop_size[MST_MAX_RESOLUTIONS];   /* any positive hop, beyond fft_size too */
    int32_t win_length[MST_MAX_RESOLUTIONS]; /* 1..fft_size; periodic Hann (a one-point window is [1]), centre-padded to fft_size */
    float w_sc, w_log_mag, w_lin_mag;        /* auraloss defaults 1, 1, 0 */
    int32_t sc_per_example;                  /* 1: mean over rows of per-row norm ratios (0.4.0); 0: global ratio */
    float eps;                               /* clamp of |X|^2, 1e-8 */
} mst_mrstft_desc;

/* Twiddle + window tables: built once per descriptor into caller memory, read-only afterwards. */
size_t mst_mrstft_tables_bytes(const mst_mrstft_desc* d);
int mst_mrstft_init_tables(const mst_mrstft_desc* d, void* tables, void* stream);
/* Per-call scratch; forward leaves what backward needs in it: the partial sums and coefficients, and - for the reference's
 * resolutions (512 / 2048 / 8192 points, hop = n_fft / 2) - the prediction's spectrum and the target's clamped magnitudes of every
 * bin and frame (12 bytes each; ~9.6 MB per row of 262144 samples): the backward reads them instead of transforming again, and
 * touches `pred` / `target` only on the generic path (other resolutions; rows that are not whole hops or shorter than two transforms;
 * every 8192-point resolution after the first - and as soon as one resolution is generic, the whole backward is). */
size_t mst_mrstft_workspace_bytes(const mst_mrstft_desc* d);
/* loss: one fp32 on the device. */
int mst_mrstft_forward(const mst_mrstft_desc* d, const float* pred, const float* target, const void* tables,
                       float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* The same loss with NOTHING kept for a backward (ABI v8): the spectra / magnitude planes are not written (153 MB per call at BASELINE
 * cfg #2), the workspace afterwards holds no valid backward state - for callers that only want the value (validation loops,
 * torch.no_grad()).  Same workspace size. */
int mst_mrstft_forward_eval(const mst_mrstft_desc* d, const float* pred, const float* target, const void* tables,
                            float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* Sharded evaluation (the batch rows are split over ranks, one process per GPU; reference: DDP over the batch axis,
 * configs/config.yaml:34-42).  Every term of the loss is a mean over rows except the batch-global spectral-convergence
 * ratio (sc_per_example = 0), whose two squared norms must be summed over ALL ranks before the division:
 *   mst_mrstft_forward_partial   transforms + reductions of this rank's rows; totals (n_res, 4) float64 on the device =
 *                                {sum (|Y|-|X|)^2, sum |Y|^2, sum |log|X| - log|Y||, sum ||X| - |Y||} per resolution
 *   (the caller all-reduces `totals` over the ranks - SUM - into global_totals)
 *   mst_mrstft_forward_finish    loss of this rank = global ratio + this rank's mean terms, so that the MEAN of the rank
 *                                losses is the single-process loss over the global batch; the backward coefficients carry
 *                                `world` on the ratio term (the adjoint of the all-reduce), so that gradients averaged over
 *                                ranks (DDP) equal the single-process gradients.  global_totals = NULL, world = 1: plain
 *                                local evaluation, identical to mst_mrstft_forward. */
int mst_mrstft_forward_partial(const mst_mrstft_desc* d, const float* pred, const float* target, const void* tables,
                               double* totals, void* workspace, size_t workspace_bytes, void* stream);
int mst_mrstft_forward_finish(const mst_mrstft_desc* d, const double* global_totals, int32_t world, float* loss,
                              void* workspace, size_t workspace_bytes, void* stream);
/* grad_loss: one fp32 on the device (dL/dloss); grad_pred (rows, n_samples) is overwritten. */
int mst_mrstft_backward(const mst_mrstft_desc* d, const float* pred, const float* target, const void* tables,
                        const float* grad_loss, float* grad_pred, void* workspace, size_t workspace_bytes,
                        void* stream);
/* Per-item losses (added at ABI v13, additive): the rows are `items` groups of R = rows / items consecutive rows, item-major (item b
 * owns rows b R .. b R + R - 1: R = 2 for a stereo item, 2 S for an item of S stereo sections), and losses[b] is what
 * mst_mrstft_forward returns for item b's rows alone - every mean over R rows, the batch-global ratio (sc_per_example = 0) over the
 * item's rows, no 1 / items anywhere, so neither in a gradient.  The transform launches are those of mst_mrstft_forward; the reduction
 * behind them folds in a fixed order (an item's rows ascending, then its resolutions ascending), so equal inputs give equal bits, and
 * items = 1 gives mst_mrstft_forward's bits.  An item's loss and gradient rows depend on that item's rows only (a NaN stays in its
 * item).  items < 1 or rows % items != 0: hipErrorInvalidValue before any launch.  Descriptor, tables and workspace (size included)
 * are those of the scalar calls.
 *   mst_mrstft_forward_items        losses: `items` fp32 on the device; leaves what mst_mrstft_backward_items needs
 *   mst_mrstft_forward_items_eval   the same values with nothing kept for a backward (as mst_mrstft_forward_eval)
 *   mst_mrstft_backward_items       grad_losses: `items` fp32 on the device, item b's cotangent reaches item b's rows only (each backward
 *                                   coefficient times its item's cotangent is one fp32 product, as in mst_mrstft_backward);
 *                                   grad_pred (rows, n_samples) is overwritten */
int mst_mrstft_forward_items(const mst_mrstft_desc* d, int32_t items, const float* pred, const float* target, const void* tables,
                             float* losses, void* workspace, size_t workspace_bytes, void* stream);
int mst_mrstft_forward_items_eval(const mst_mrstft_desc* d, int32_t items, const float* pred, const float* target, const void* tables,
                                  float* losses, void* workspace, size_t workspace_bytes, void* stream);
int mst_mrstft_backward_items(const mst_mrstft_desc* d, int32_t items, const float* pred, const float* target, const void* tables,
                              const float* grad_losses, float* grad_pred, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * batch_stereo_peak_normalize (reference mst/utils.py:14-29): y = x / clamp(max_{ch,t}|x|, 1e-8)
 * per batch item; x, y, grads are dense (bs, 2, n_samples).  The workspace written by forward is
 * what backward reads (peak and arg-max per batch item). */
size_t mst_peak_normalize_workspace_bytes(int32_t bs, int64_t n_samples);
int mst_peak_normalize_forward(const float* x, float* y, int32_t bs, int64_t n_samples, void* workspace,
                               size_t workspace_bytes, void* stream);
int mst_peak_normalize_backward(const float* x, const float* grad_y, float* grad_x, int32_t bs, int64_t n_samples,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Integrated loudness (ITU-R BS.1770-4 as pyloudnorm.Meter(rate).integrated_loudness computes it with its defaults: K-weighting,
 * 0.4 s gating blocks with 75 % overlap, absolute gate -70 LUFS, relative gate -10 LU) - the meter the reference's inference
 * driver, data pipeline and evaluation scripts normalise with (mst/utils.py:67,93; mst/dataloader.py:66).  PARITY UNPINNED: a
 * restatement of pyloudnorm's published source, not checked against the package.
 *   x               `rows` signals of `channels` (1..5, weights 1 1 1 1.41 1.41) channels of n_samples fp32 samples, unit sample
 *                   stride, row_stride / channel_stride elements between rows / channels (a last-dimension crop needs no copy)
 *   tables          mst_loudness_tables_bytes(rate) bytes filled once by mst_loudness_init_tables(rate); they open with 4096 int32
 *                   block boundaries  bound[k] = int(0.4 * (k * 0.25) * rate)  evaluated on the host in float64 exactly as
 *                   pyloudnorm writes it (gating block j = samples [bound[j], bound[j + 4])), followed by the filter coefficients
 *                   and the powers of the filter's state-transition matrix
 *   lufs            (rows) fp32; -inf when no block passes the gates
 *   block_loudness  NULL or (rows, mst_loudness_num_blocks(n_samples, rate)) fp32, the loudness l_j of every gating block
 * mst_loudness_num_blocks / mst_loudness_workspace_bytes return 0 for what is not supported: signals shorter than one gating
 * block (pyloudnorm raises there; n_samples == 0.4 * rate is one block), more than 4092 blocks, sample rates below 20500 Hz.
 * Four launches, deterministic (no floating-point atomics), no host synchronisation. */
size_t mst_loudness_tables_bytes(int32_t sample_rate);
int mst_loudness_init_tables(int32_t sample_rate, void* tables, void* stream);
int32_t mst_loudness_num_blocks(int64_t n_samples, int32_t sample_rate);
size_t mst_loudness_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate);
int mst_loudness_integrated(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride,
                            int64_t channel_stride, int32_t sample_rate, const void* tables, float* lufs, float* block_loudness,
                            void* workspace, size_t workspace_bytes, void* stream);
/* y[row] = x[row] * 10^((target_lufs - lufs[row]) / 20), the gain formed on the device; x strided as above, y dense
 * (rows, channels, n_samples).  keep (rows) bytes or NULL: 1 where lufs[row] >= floor_lufs and finite (-inf floor: every row
 * that has a loudness); rows that are not kept are written as zeros. */
int mst_loudness_normalize(const float* x, float* y, const float* lufs, int32_t rows, int32_t channels, int64_t n_samples,
                           int64_t row_stride, int64_t channel_stride, float target_lufs, float floor_lufs, uint8_t* keep,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Windowed loudness (an addition to ABI v13): the gated loudness of every window of a song, from ONE pass of the meter.
 *   complete block  gating block j is complete when bound[j + 4] <= n_samples; there are NB = floor((n - 0.4 rate) / (0.1 rate)) + 1
 *                   of them (at most MST_LOUDNESS_MAX_BLOCKS).  The clipped partial last block pyloudnorm appends is not used here.
 *   window w        the blocks w * hop_blocks .. w * hop_blocks + window_blocks - 1; NW = floor((NB - window_blocks) / hop_blocks) + 1
 *                   windows.  It covers the samples [bound[w * hop_blocks], bound[w * hop_blocks + window_blocks + 3]).
 *   its loudness    BS.1770 gating over exactly those blocks, every sum in float64: absolute gate l_j >= -70, Gamma_r from the mean
 *                   of the survivors minus 10, final set l_j > Gamma_r and l_j > -70, -0.691 + 10 log10(sum_c G_c mean z_c); -inf
 *                   when the final set is empty.  The block energies are those of the song filtered once - the K-weighting is warm
 *                   at a window's start: this is the loudness of the window as part of the song, not of the crop filtered from rest.
 *   window_lufs     (rows, NW) fp32
 *   lufs            NULL or (rows) fp32: the whole signal's loudness, bit for bit what mst_loudness_integrated writes
 * The boundary table must be equally spaced, bound[k] == k * bound[1] for every k of the table (44100, 48000, 22050, 32000, 96000,
 * 88200, 24000 Hz are; 44101 Hz is not).  Any other rate, window_blocks or hop_blocks < 1, window_blocks > NB and whatever
 * mst_loudness_workspace_bytes refuses is refused: mst_loudness_windows_workspace_bytes returns 0, and mst_loudness_num_windows -
 * a status like every entry that is not a size - writes 0 windows and returns an error.  num_windows is a host pointer.
 * x, the strides and the tables are mst_loudness_integrated's.  Its four launches and one more (k_loud_windows, one wave per window
 * and row, fixed-order sums); deterministic, no host synchronisation, nothing relies on a cleared workspace. */
#define MST_LOUDNESS_MAX_BLOCKS 4092
int mst_loudness_num_windows(int64_t n_samples, int32_t sample_rate, int32_t window_blocks, int32_t hop_blocks, int32_t* num_windows);
size_t mst_loudness_windows_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate,
                                            int32_t window_blocks, int32_t hop_blocks);
int mst_loudness_windows(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride, int64_t channel_stride,
                         int32_t sample_rate, const void* tables, int32_t window_blocks, int32_t hop_blocks, float* window_lufs,
                         float* lufs, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The rest of a delivery meter (additions to ABI v13): true peak, short-term loudness, loudness range, and a normalisation
 * that respects a true-peak ceiling.  PARITY UNPINNED: written from the published definitions (BS.1770-4 Annex 2, EBU Tech 3341 /
 * 3342, libebur128's interpolator), never run against another meter.
 *
 * True peak of an item x (channels, n), oversampling factor F = 4 below 96000 Hz, 2 from 96000 Hz to below 192000 Hz (anything else is
 * refused: mst_true_peak_factor - a status like every entry that is not a size - writes 0 and returns an error; factor is a host pointer):
 *   h[j] = sinc((j - 24) / F) * 0.5 * (1 - cos(2 pi j / 48)), j = 0..48, float64 on the host, rounded once to fp32; the sinc is exact
 *          at whole arguments, so phase 0 is the identity (h[24] = 1, exact zeros) and the sample peak is always contained.
 *          mst_true_peak_coefficients (host only) returns the 49 fp32 taps the kernel uses.
 *   y[k] = sum_j h[j] xz[(k - j) / F] over the j with (k - j) % F == 0, xz = x extended by zeros, k = 0 .. F (n - 1) + 48: the FULL
 *          convolution - the samples after the last input count, which libebur128 (it never flushes its delay line) leaves out; the
 *          result does not depend on where the signal sits in a buffer.
 *   TP   = max over channels and k of |y|, fp32 fused multiply-adds in a fixed tap order (at F = 2 two halves of 12 taps, added).
 *          Silence gives 0, a NaN in an item makes that item's result NaN (and no other's), an infinity gives +inf.
 *   true_peak (rows) LINEAR fp32 (20 log10 of it is dBTP); channel_peak NULL or (rows, channels).
 * x: unit sample stride, row_stride / channel_stride elements, any 4-byte alignment.  rows * channels <= 65535, n_samples >= 1.  Two
 * launches (one workgroup per MST_TRUE_PEAK_TILE positions and signal, then one wave per row), no atomics, deterministic; the
 * interpolated signal is never written; nothing relies on a cleared workspace. */
#define MST_TRUE_PEAK_TILE 2048
int mst_true_peak_factor(int32_t sample_rate, int32_t* factor);
int mst_true_peak_coefficients(int32_t factor, float* h49);
size_t mst_true_peak_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t factor);
int mst_true_peak(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride, int64_t channel_stride,
                  int32_t factor, float* true_peak, float* channel_peak, void* workspace, size_t workspace_bytes, void* stream);
/* The same two launches, also writing sample_peak NULL | (rows) linear fp32: max |x| over the item, which is phase 0 of the interpolator
 * and falls out of the same pass (a meter report shows it beside the true peak).  NaN rule as above; same workspace. */
int mst_true_peak_sample(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride, int64_t channel_stride,
                         int32_t factor, float* true_peak, float* channel_peak, float* sample_peak, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Short-term loudness and loudness range (EBU Tech 3342), from the meter's ONE K-weighting pass.  With step = rate / 10 (the equally
 * spaced boundary table mst_loudness_windows needs; other rates are refused) a signal has NSEG = n / step complete segments:
 *   short-term window k  the samples [bound[k H], bound[k H + 30]) = 3 s, H = hop_segments in 1..30; NS = (NSEG - 30) / H + 1 windows;
 *                        E_k = sum_c G_c (sum of the K-weighted y^2 over the window) / (30 step), l_k = -0.691 + 10 log10 E_k, ungated
 *   range                absolute gate l_k >= -70; relative gate l_k >= -20 + loudness of the mean E_k of the absolutely gated windows;
 *                        the m survivors in ascending order of energy: lo = element ((m - 1) * 10 + 50) / 100, hi = element
 *                        ((m - 1) * 95 + 50) / 100 (integers); LRA = l(hi) - l(lo), 0 when m == 0.  All in float64, fixed order.
 *   short_term_lufs NULL or (rows, NS); range_lu (rows); range_bounds NULL or (rows, 2) = l(lo), l(hi) (NaN when m == 0);
 *   lufs NULL or (rows) and block_loudness NULL or (rows, num_blocks): bit for bit what mst_loudness_integrated writes.
 * A signal shorter than 3 s, H outside 1..30 and whatever mst_loudness_workspace_bytes refuses are refused
 * (mst_loudness_range_workspace_bytes returns 0; mst_loudness_num_short_term writes 0 through its host pointer and returns an error).
 * The meter's four launches and one more (k_loud_range, one workgroup per row). */
int mst_loudness_num_short_term(int64_t n_samples, int32_t sample_rate, int32_t hop_segments, int32_t* count);
size_t mst_loudness_range_workspace_bytes(int32_t rows, int32_t channels, int64_t n_samples, int32_t sample_rate, int32_t hop_segments);
int mst_loudness_range(const float* x, int32_t rows, int32_t channels, int64_t n_samples, int64_t row_stride, int64_t channel_stride,
                       int32_t sample_rate, const void* tables, int32_t hop_segments, float* short_term_lufs, float* range_lu,
                       float* range_bounds, float* lufs, float* block_loudness, void* workspace, size_t workspace_bytes, void* stream);
/* mst_loudness_normalize with the gain capped at a true-peak ceiling: g = min(10^((target_lufs - lufs[row]) / 20),
 * 10^(ceiling_dbtp / 20) / true_peak[row]), formed on the device from the two buffers (true_peak LINEAR, as mst_true_peak writes it).
 * gain_db (rows): the gain that was applied, ceiling_dbtp - 20 log10(true_peak) where the cap took hold, target_lufs - lufs elsewhere,
 * -inf for a row that is not kept.  keep and the zero rows are mst_loudness_normalize's. */
int mst_loudness_normalize_limited(const float* x, float* y, const float* lufs, const float* true_peak, int32_t rows, int32_t channels,
                                   int64_t n_samples, int64_t row_stride, int64_t channel_stride, float target_lufs, float floor_lufs,
                                   float ceiling_dbtp, float* gain_db, uint8_t* keep, void* stream);

/* The section picker (csrc/mst_sections.hip): which windows of a song a sectioned fit should see, so that every track plays
 * in one of them.  One workgroup, deterministic, never waits on the host.
 *   track_lufs (n_tracks, n_windows) fp32, mix_lufs (n_windows): windowed loudness of the tracks and of their mix
 *   active[t][w]  = track_lufs[t][w] >= track_floor[t]   (NaN and -inf are not active, by the comparison)
 *   eligible[w]   = mix_lufs[w] >= mix_floor and some track is active in w
 *   round r = 0 .. count - 1: the candidates are the eligible w with |w - c| >= min_gap for every window c chosen so far; the one with
 *   the lexicographically largest (new[w], act[w], mix_lufs[w], -w) is taken - new[w] the number of active tracks not yet covered,
 *   act[w] the number of active tracks - and its active tracks become covered.  When no candidate is left, this and every later
 *   entry of `windows` is -1 and its row of `active` zero.
 *   windows (count) int32; active (count, n_tracks) bytes, row r = active[:, windows[r]]; covered (n_tracks) bytes
 * n_tracks 1..MST_PICK_MAX_TRACKS, n_windows 1..MST_LOUDNESS_MAX_BLOCKS, count 1..MST_OPT_MAX_SECTIONS (what
 * mst_logit_adam_step_sections takes), min_gap >= 1: anything else is an error status and no launch. */
#define MST_PICK_MAX_TRACKS 256
#define MST_OPT_MAX_SECTIONS 64
int mst_pick_sections(const float* track_lufs, const float* mix_lufs, const float* track_floor, float mix_floor, int32_t n_tracks,
                      int32_t n_windows, int32_t count, int32_t min_gap, int32_t* windows, uint8_t* active, uint8_t* covered,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Sample-rate conversion (ABI v11) with the semantics of torchaudio.functional.resample(x, orig_freq, new_freq) at its defaults
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) - what every script of the reference applies to the tracks and the
 * reference mix before anything else (scripts/run.py:78-79, scripts/online.py:223-226, mst/callbacks/mix.py:52).  PARITY UNPINNED: a
 * restatement of torchaudio's published source, not checked against the package.  With o = orig / gcd, n = new / gcd:
 *   y[j n + i] = sum_k h[i][k] xpad[j o + k],  h in float64 as torchaudio writes it, rounded once to fp32; only taps whose fp32
 *   value is exactly 0 are skipped.  n_out = mst_resample_out_samples = ceil(n n_samples / o), in integers (torchaudio evaluates
 *   this through a float32 tensor, which can differ by one sample above 2^24 output samples; that is not imitated).
 *   x        `rows` signals of n_samples fp32 samples, unit sample stride, row_stride elements apart, any 4-byte alignment
 *   tables   mst_resample_tables_bytes(orig, new) bytes filled once by mst_resample_init_tables.  They open with 16 int32 words:
 *            o, n, width, T (taps per output), frames per tile of the forward (a tile is that many x n consecutive outputs, staged
 *            and computed as one piece by a workgroup), E (taps per input sample of the adjoint), frames per tile of the adjoint
 *            (x o input samples), the word offsets of the two coefficient tables; the rest is reserved
 *   y        dense (rows, n_out), every sample written once
 * mst_resample_backward is the adjoint: grad_y dense (rows, n_out) -> grad_x dense (rows, n_samples), from the same fp32
 * coefficients.  Supported: reduced o, n <= 1024, o != n (equal rates are the identity: mst_resample_out_samples returns n_samples
 * and there is nothing to launch), at most 132 taps per output (o / n up to ~10.8), 1 <= n_samples <= 2^40; otherwise
 * mst_resample_tables_bytes and mst_resample_out_samples return 0 and the launchers refuse.  One launch per call, deterministic (no
 * atomics), a row's result does not depend on the other rows, no host synchronisation. */
size_t mst_resample_tables_bytes(int32_t orig_freq, int32_t new_freq);
int mst_resample_init_tables(int32_t orig_freq, int32_t new_freq, void* tables, void* stream);
int64_t mst_resample_out_samples(int64_t n_samples, int32_t orig_freq, int32_t new_freq);
int mst_resample_forward(const float* x, int32_t rows, int64_t n_samples, int64_t row_stride, int32_t orig_freq, int32_t new_freq,
                         const void* tables, float* y, void* stream);
int mst_resample_backward(const float* grad_y, int32_t rows, int64_t n_samples, int32_t orig_freq, int32_t new_freq,
                          const void* tables, float* grad_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-song mix optimisation (ABI v12): the bookkeeping of one iteration of the loop in the reference's scripts/online.py:71-106 -
 * console parameters p = sigmoid(theta), torch.optim.Adam on the logits theta - as ONE launch, so that a loop of console forward,
 * loss, backward and this step never waits for the host.  PARITY UNPINNED: a restatement of torch.optim.Adam (single-tensor path at
 * its defaults: no weight decay, no amsgrad, not maximising) and torch.sigmoid from torch's published source.
 *   segments     host array of 1..MST_OPT_MAX_SEGMENTS parameter tensors (copied into the launch, need not outlive the call).  Per
 *                segment, all device pointers, dense fp32, `count` elements, caller-owned:
 *                  theta   the logits, updated in place
 *                  p       sigmoid(theta): written by mst_logit_adam_init, read (as the value the forward consumed) and rewritten
 *                          by mst_logit_adam_step
 *                  grad_p  dL/dp, read-only, or NULL: a parameter without gradient, which keeps theta, its moments and p bit for
 *                          bit (torch skips a parameter whose .grad is None)
 *   state        mst_logit_adam_state_bytes(sum of the counts) bytes, caller-owned, opaque but for its first four int32 words:
 *                  [0] t, the number of updates applied   [1] status, 0 or MST_OPT_STATUS_NONFINITE, sticky
 *                  [2] the index of the iteration that set the status   [3] the number of mst_logit_adam_step calls so far
 *                followed by 12 reserved words, the fp32 first moments of all segments in segment order, then their second
 *                moments.  The bias corrections
 *                1 - beta^t are formed from t in float64 and rounded once; nothing else is kept for them.
 *                mst_logit_adam_init zeroes the block; mst_logit_adam_state_bytes returns 0 for a count outside [1, 2^20].
 *   loss_terms   host array of 1..MST_OPT_MAX_TERMS device pointers to fp32 scalars
 *   history_row  device, 1 + n_terms fp32: [0] the sum of the terms, added left to right in fp32 from zero, [1 + k] term k
 * One step, per coordinate:  g = dp p (1 - p);  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g^2;  t += 1;
 * theta -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  p = sigmoid(theta).  If a loss term or an element of a
 * gradient is not finite, the history row is still written and [3] advances, but no coordinate changes, t stays, and the first such
 * iteration is recorded in [1], [2]: the caller reads them when the loop is over.  The step reads nothing from the host - the step
 * count lives in the state - and the same arguments (but history_row) serve every iteration.  One workgroup, one launch per call on
 * `stream`, deterministic, no host synchronisation; every buffer is written exactly up to its count.  Bad arguments (NULL theta /
 * p / state / history_row, counts or numbers of segments / terms out of range, lr <= 0, a beta outside [0, 1), eps < 0) return
 * non-zero before anything is launched. */
#define MST_OPT_MAX_SEGMENTS 4
#define MST_OPT_MAX_TERMS 8
#define MST_OPT_STATUS_NONFINITE 1
typedef struct mst_logit_adam_segment {
    float* theta;
    float* p;
    const float* grad_p;
    int64_t count;
} mst_logit_adam_segment;
size_t mst_logit_adam_state_bytes(int64_t n_params);
int mst_logit_adam_init(const mst_logit_adam_segment* segments, int32_t n_segments, void* state, void* stream);
int mst_logit_adam_step(const mst_logit_adam_segment* segments, int32_t n_segments, const float* const* loss_terms, int32_t n_terms,
                        float* history_row, double lr, double beta1, double beta2, double eps, void* state, void* stream);

/* Batched fits: `items` independent optimisations (random restarts, one song against several references, several songs against one)
 * in ONE launch of `items` workgroups.  Workgroup b is mst_logit_adam_step on item b - the same operations in the same order, so
 * item b's logits, p, moments, t and history row are bit-identical to a single-song session fed item b's gradients - and exchanges
 * nothing with the others.
 *   segments      as above, with `count` the total over all items: it must divide by `items`, and item b owns elements
 *                 [b count/items, (b + 1) count/items) of theta, p and grad_p - the leading batch dimension of a dense (items, ...) tensor
 *   state         mst_logit_adam_batch_state_bytes(items, params_per_item) bytes, params_per_item = sum of count/items.  Item b's block
 *                 starts at int32 word b (16 + 2 params_per_item) and has the layout of the single call: words [0..3] t, status,
 *                 the iteration that set it, the number of calls; 12 reserved words; item b's first moments in segment order; its
 *                 second moments.  mst_logit_adam_init_batch zeroes every block and writes p = sigmoid(theta).
 *   loss_terms    device, dense (items, n_terms) fp32: row b is item b's terms
 *   history_rows  device, dense (items, 1 + n_terms) fp32: row b is item b's history row of this iteration
 * A loss term or gradient element of item b that is not finite stops item b's update for this iteration and is recorded in item
 * b's words [1], [2]; no other item is affected.  1 <= items <= 1024, 1 <= params_per_item <= 2^20: anything else (and every bad
 * argument of the single call) returns 0 / non-zero before anything is launched. */
size_t mst_logit_adam_batch_state_bytes(int32_t items, int64_t params_per_item);
int mst_logit_adam_init_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, void* state, void* stream);
int mst_logit_adam_step_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, const float* loss_terms,
                              int32_t n_terms, float* history_rows, double lr, double beta1, double beta2, double eps, void* state,
                              void* stream);

/* The same steps, keeping the best iterate on the device and freezing an item that has stopped improving.  Still ONE
 * launch per call, one workgroup per item, nothing read by the host.  `state` is the block of the calls above, with their layout, set
 * up by mst_logit_adam_init / _init_batch; none of its reserved words is used.  `best` is a second caller-owned block of
 * mst_logit_adam_best_bytes(items, params_per_item) bytes (items = 1 for the single call) that the caller fills with zeros: all zero
 * means "no best yet".  Item b's part starts at int32 word b (16 + params_per_item + 1 + MST_OPT_MAX_TERMS):
 *   [0] the best iteration + 1, 0 = none     [1] the best loss, fp32 bits     [2] iterations since the last improvement
 *   [3] the iteration at which the item settled + 1, 0 = still running        [4..15] reserved, left zero
 *   then params_per_item fp32: the item's logits at the best iteration, in segment order, NULL-gradient segments included
 *   then 1 + n_terms fp32: that iteration's history row (the block leaves room for 1 + MST_OPT_MAX_TERMS)
 * One call for one item, with n = state word [3] on entry and L the fp32 loss sum that goes to history_row[0]:
 *   settled (best[3] != 0)   the history row is written and state word [3] advances; theta, p, the moments, t, the status words and
 *                            the best block stay as they are
 *   not finite               exactly the plain step (row written, status recorded, nothing updated); the best block, its wait count
 *                            included, is not touched
 *   otherwise                the iteration improves if there is no best yet or L < fl32(best loss - fl32(min_delta)) - one fp32
 *                            subtraction and a strict <: a loss exactly min_delta below the best is no improvement and a tie keeps the
 *                            earlier iterate.  On an improvement L, n, the history row and theta AS IT IS BEFORE THIS CALL'S UPDATE (the
 *                            logits the loss was evaluated at) are stored and the wait count becomes 0; otherwise the wait count grows
 *                            by one.  Then the update of the plain step, the same operations in the same order: theta, p, the moments,
 *                            t and the history row are bit-identical to mst_logit_adam_step's on the same inputs.  Then, if
 *                            patience > 0 and the wait count has reached it, n + 1 goes to [3]: the item is frozen from its next call on.
 * patience = 0 never freezes.  Refused before anything is launched, besides what the plain calls refuse: a NULL or misaligned `best`,
 * min_delta negative or not finite (as fp32 too), patience < 0.  mst_logit_adam_best_bytes returns 0 for sizes out of range. */
size_t mst_logit_adam_best_bytes(int32_t items, int64_t params_per_item);
int mst_logit_adam_step_best(const mst_logit_adam_segment* segments, int32_t n_segments, const float* const* loss_terms,
                             int32_t n_terms, float* history_row, double lr, double beta1, double beta2, double eps, double min_delta,
                             int32_t patience, void* state, void* best, void* stream);
int mst_logit_adam_step_best_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, const float* loss_terms,
                                   int32_t n_terms, float* history_rows, double lr, double beta1, double beta2, double eps,
                                   double min_delta, int32_t patience, void* state, void* best, void* stream);

/* One parameter set fitted to SEVERAL SECTIONS of a song at once: the console runs at batch `sections` with parameter
 * leaves whose rows are equal, autograd hands back one gradient row per section, and the step sums them.  Per segment `theta` has
 * `count` elements as above, while `p` and `grad_p` are dense (sections, count): row r starts r * count elements in.
 *   mst_logit_adam_init_sections  zeroes the state block and writes sigmoid(theta) to EVERY row of p
 *   mst_logit_adam_step_sections  dp[i] = ((g_0[i] + g_1[i]) + g_2[i]) + ... in fp32 in row order, then the step of
 *                                 mst_logit_adam_step on dp - the same operations in the same order, reading p from row 0 - and the
 *                                 new p[i] written to every row.  A NULL grad_p keeps theta, the moments and all rows of p.
 * A gradient element OR a partial sum that is not finite (two finite addends may overflow) stops the iteration exactly as a non-finite
 * gradient stops mst_logit_adam_step.  `best` NULL: the plain step, min_delta and patience are not looked at.  `best` non-NULL: the
 * step of mst_logit_adam_step_best with that block, min_delta and patience.  state and best keep the single call's layouts and sizes:
 * mst_logit_adam_state_bytes(sum of the counts), mst_logit_adam_best_bytes(1, sum of the counts).  sections = 1 gives the bits of
 * mst_logit_adam_init / _step / _step_best in every output.  One workgroup, one launch, no host synchronisation.  sections outside
 * [1, 64] and every bad argument of the single calls return non-zero before anything is launched. */
int mst_logit_adam_init_sections(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t sections, void* state,
                                 void* stream);
int mst_logit_adam_step_sections(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t sections,
                                 const float* const* loss_terms, int32_t n_terms, float* history_row, double lr, double beta1, double beta2,
                                 double eps, double min_delta, int32_t patience, void* state, void* best, void* stream);

/* A BATCH of sectioned fits: `items` parameter sets with `sections` gradient rows each, in ONE launch of `items`
 * workgroups - restarts of a sectioned fit, one sectioned song against several references.  Workgroup b is
 * mst_logit_adam_step_sections on item b, the same operations in the same order, and exchanges nothing with the others.  Per segment
 *   theta           `count` = items * c elements, item-major, as in the batch calls: item b owns [b c, (b + 1) c)
 *   p, grad_p       dense (items, sections, c): row item * sections + r is section r of `item` - the item-major order of the pooled
 *                   loss calls below and of a console that runs at batch items * sections
 *   state, best     mst_logit_adam_batch_state_bytes(items, sum of c), mst_logit_adam_best_bytes(items, sum of c): the batch layouts
 *   loss_terms      device, dense (items, n_terms) fp32;  history_rows  device, dense (items, 1 + n_terms) fp32
 * Item b's gradient at a coordinate is ((g_0 + g_1) + g_2) + ... over ITS rows in fp32; p is read from its row 0 and the new p goes
 * to all of its rows.  A non-finite addend, partial sum or loss term of item b stops item b's iteration alone.  `best` NULL: the plain
 * step; non-NULL: the best-iterate step per item, as in mst_logit_adam_step_best_batch.  items = 1 gives the bits of the _sections
 * calls, sections = 1 those of the _batch calls, in every output.  items outside [1, 1024], sections outside [1, 64], a count that
 * `items` does not divide and every bad argument of those calls return non-zero before anything is launched. */
int mst_logit_adam_init_sections_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                                       void* state, void* stream);
int mst_logit_adam_step_sections_batch(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                                       const float* loss_terms, int32_t n_terms, float* history_rows, double lr, double beta1,
                                       double beta2, double eps, double min_delta, int32_t patience, void* state, void* best,
                                       void* stream);

/* LINKED ROWS: the calls above for a fit in which groups of rows of one segment share one set of logits - the two
 * channels of a stereo stem that the loaders split into two mono rows.  Per item that segment is dense (rows, cols); the members of a
 * group are its rows in ascending order, the first is its leader, and leader[r] names the leader of row r.  At `mirror_col` a
 * follower's logit is MINUS its leader's: sigmoid(-x) = 1 - sigmoid(x), the pan of the other channel.  The map is copied into the
 * launch (it need not outlive the call) and is shared by all items.  `items`, `sections`, a nullable `best` and every other argument
 * keep the meaning, layouts and sizes of mst_logit_adam_init_sections_batch / _step_sections_batch.
 *   mst_logit_adam_init_linked  theta[f, c] <- theta[l, c] for every follower row f of leader l, -theta[l, c] at mirror_col (the
 *                               negation is exact); then the state block zeroed and sigmoid(theta) written to every row of p
 *   mst_logit_adam_step_linked  for the tied segment only the lane of a leader coordinate (l, c) acts.  Per member m: d_m the section
 *                               sum over m's rows, g_m = (d_m (1 - p_m)) p_m with p_m from m's own row 0, negated for a follower at
 *                               mirror_col; G = ((g_m0 + g_m1) + ...) in fp32 in member order; the Adam statements of
 *                               mst_logit_adam_step on G for the leader's moments and logit; then theta, p = sigmoid of the member's
 *                               own logit, and (on an improvement) the best block's logits before the update, for every member and
 *                               every section row.  Followers' moment words stay zero.  An addend or a partial sum of G that is not
 *                               finite stops the item's iteration like any non-finite gradient.  The other segments, and the tied one
 *                               when its grad_p is NULL, take the path of the calls above.
 * A map in which every row leads itself gives the bits of mst_logit_adam_init_sections_batch / _step_sections_batch in every output.
 * A NULL `links`, a segment that is not in the table, rows outside [1, MST_OPT_MAX_LINK_ROWS], rows * cols different from the
 * segment's per-item count, a leader[r] > r or one that does not lead itself, mirror_col outside [-1, cols) and every bad argument of
 * the calls above return non-zero before anything is launched. */
#define MST_OPT_MAX_LINK_ROWS 256
typedef struct mst_logit_adam_links {
    int32_t segment;    /* which segment is tied (the track tensor: 0) */
    int32_t rows, cols; /* per item that segment is dense (rows, cols); rows * cols == its per-item count */
    int32_t mirror_col; /* a follower's logit in this column is MINUS its leader's; -1: none */
    uint8_t leader[MST_OPT_MAX_LINK_ROWS]; /* leader[r] <= r, leader[leader[r]] == leader[r]; leader[r] == r: r leads itself */
} mst_logit_adam_links;
int mst_logit_adam_init_linked(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                               const mst_logit_adam_links* links, void* state, void* stream);
int mst_logit_adam_step_linked(const mst_logit_adam_segment* segments, int32_t n_segments, int32_t items, int32_t sections,
                               const mst_logit_adam_links* links, const float* loss_terms, int32_t n_terms, float* history_rows,
                               double lr, double beta1, double beta2, double eps, double min_delta, int32_t patience, void* state,
                               void* best, void* stream);

/* ------------------------------------------------------------------------------------------
 * AudioFeatureLoss (reference mst/loss.py:198-260): five weighted MSE terms between features of
 * pred and target, both dense (bs, 2, n_samples): rms, crest factor, stereo width, stereo imbalance
 * (:127-195) and the 24-band Bark spectrum of mid/side (:62-124; STFT 32768 / hop 8192 / Hann).
 *   weights5     host array of the five weights, in that order
 *   filterbank   device (16385, 24) fp32 = barkscale_fbanks(16385, 20, 20000, 24, sample_rate)
 *                (reference mst/filter.py:107-161; a constant table built by the host wrapper)
 *   losses5      device, the five weighted losses in the reference's key order */
size_t mst_afloss_tables_bytes(void);
int mst_afloss_init_tables(void* tables, void* stream);
size_t mst_afloss_workspace_bytes(int32_t bs, int64_t n_samples);
int mst_afloss_forward(const float* pred, const float* target, int32_t bs, int64_t n_samples, const float* weights5,
                       const void* tables, const float* filterbank, float* losses5, void* workspace,
                       size_t workspace_bytes, void* stream);
/* grad_losses5: device, dL/d(loss_k); grad_pred (bs, 2, n_samples) is overwritten. */
int mst_afloss_backward(const float* pred, const float* target, int32_t bs, int64_t n_samples, const float* weights5,
                        const void* tables, const float* filterbank, const float* grad_losses5, float* grad_pred,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Feature profiles (ABI v13): none of the five features depends on the length of the signal, so the target may be ANALYSED ONCE into
 * 54 float64 numbers per batch item and the loss and its backward then run against those instead of against audio - the target may
 * have any length > 16384 (the reference accepts unequal lengths, mst/loss.py:127-260), it need not stay resident, and a loop against
 * one fixed target transforms 2 bs signals per forward instead of 4 bs.
 *
 * Layout of a profile row (MST_AF_PROFILE_DOUBLES doubles; fixed: stored profiles stay readable, a later quantity is appended under
 * a new count).  The length of the analysed signal is NOT part of it.
 *   [0..3]    mean L^2, mean R^2, mean (L+R)^2, mean (L-R)^2   float64 sums of fp32 block sums, divided by n
 *   [4..5]    max |L|, max |R|
 *   [6..29]   log(band energy + 1e-8) of the 24 Bark bands of the mid signal L+R   (fp32 values, widened)
 *   [30..53]  the same of the side signal L-R
 * From these: rms = sqrt(max([0..1], 1e-8)); crest factor = 20 log10([4..5] / rms); width = [3] / max([2], 1e-8);
 * imbalance = ([1] - [0]) / max([1] + [0], 1e-8); Bark spectrum [b][band][mid|side].
 *
 *   mst_af_profile              x (bs, 2, n_samples) -> profile (bs, 54); exactly bs*54 doubles are written
 *   mst_afloss_forward_profile  the five weighted losses of pred (bs, 2, n_samples) against profile (bs, 54)
 *   mst_afloss_backward_profile grad_pred of that call; same workspace, after the forward, as mst_afloss_backward
 * pred is analysed by the arithmetic mst_af_profile uses (same strip plan at the same bs and n_samples): the loss of a signal against
 * its own profile is exactly 0.  mst_afloss_forward / _backward above are unchanged and bit-identical to ABI v12.  Fixed-order sums,
 * no float atomics: bitwise reproducible.  n_samples <= 16384, bs <= 0, a NULL pointer or a workspace that is too small return
 * non-zero before anything is launched; the *_workspace_bytes functions return 0 for such bs / n_samples. */
#define MST_AF_PROFILE_DOUBLES 54
size_t mst_af_profile_workspace_bytes(int32_t bs, int64_t n_samples);
int mst_af_profile(const float* x, int32_t bs, int64_t n_samples, const void* tables, const float* filterbank, double* profile,
                   void* workspace, size_t workspace_bytes, void* stream);
size_t mst_afloss_profile_workspace_bytes(int32_t bs, int64_t n_samples);
int mst_afloss_forward_profile(const float* pred, const double* profile, int32_t bs, int64_t n_samples, const float* weights5,
                               const void* tables, const float* filterbank, float* losses5, void* workspace,
                               size_t workspace_bytes, void* stream);
int mst_afloss_backward_profile(const float* pred, const double* profile, int32_t bs, int64_t n_samples, const float* weights5,
                                const void* tables, const float* filterbank, const float* grad_losses5, float* grad_pred,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Per-item loss against a profile: row b of `losses` (bs, 5) is the five weighted terms of item b as if it were a batch of one (the
 * batch divisor of the mean-squared errors is 1, not bs), and row b of `grad_losses` (bs, 5) scales item b's gradient only - what a
 * batch of independent fits needs (mst_logit_adam_step_batch).  The analysis is that of mst_afloss_forward_profile: the same launches
 * and the same strip plan at (bs, n_samples); only the epilogues differ (one item per workgroup in the final kernel; the backward
 * takes the item's cotangent and the divisor 1 where the calls above take one cotangent and bs).  So bs = 1 gives the bits of
 * mst_afloss_forward_profile / _backward_profile, the mean over the items is the batch call's value to one fp32 rounding, and for a
 * power-of-two bs the gradient under an all-ones cotangent is exactly bs times the batch call's.  An item never reads another item's
 * audio, profile row or cotangent.  Workspace: mst_afloss_profile_workspace_bytes(bs, n_samples), the same size as for the batch
 * calls; the backward follows its forward on the same workspace.  Fixed-order sums, no float atomics: bitwise reproducible.  Bad
 * arguments return non-zero before anything is launched, as above. */
int mst_afloss_forward_profile_items(const float* pred, const double* profile, int32_t bs, int64_t n_samples, const float* weights5,
                                     const void* tables, const float* filterbank, float* losses, void* workspace,
                                     size_t workspace_bytes, void* stream);
int mst_afloss_backward_profile_items(const float* pred, const double* profile, int32_t bs, int64_t n_samples, const float* weights5,
                                      const void* tables, const float* filterbank, const float* grad_losses, float* grad_pred,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* Pooled sections: S sections of one signal are ONE feature row.  All five features are aggregates over time, so the
 * features of several sections taken together are formed from what the analysis leaves per section, before the nonlinear maps.
 * pred / x is (items * sections, 2, n_samples), item-major: row item * sections + s is section s of `item`; all sections share one
 * length.  Per item, from the per-section statistics and linear band energies:
 *   mean squares   (m_0 + m_1 + ... + m_{S-1}) / S in float64 in section order: the mean over all S n_samples samples
 *   peaks          the largest section peak per channel; its arg-max is a (section, sample) pair, the first in section order, then in
 *                  time order - a tie goes to the earlier section
 *   Bark bands     lin[j] = (lin_0[j] + ... + lin_{S-1}[j]) / S per signal (mid, side): the mean magnitude over all frames of all
 *                  sections (every section has the same frame count and keeps its own reflect padding), then log(lin + 1e-8).  The sum
 *                  is formed in FLOAT64 from the sections' fp32 values and rounded to fp32 once, so S = 1 gives the bits of lin.
 * In the reference's words: rms, crest factor, width and imbalance are those of torch.cat(sections, dim=-1), and the Bark term is
 * log(mean_s(exp(compute_barkspectrum(section_s)) - 1e-8) + 1e-8).
 *   mst_af_profile_pooled               x -> profile (items, 54): the pooled row in the profile layout above; items*54 doubles written
 *   mst_afloss_forward_profile_pooled   losses (items, 5): the five weighted terms of item's pooled row against profile row `item`,
 *                                       each item a batch of one as in the _items call
 *   mst_afloss_backward_profile_pooled  grad_losses (items, 5) -> grad_pred (items * sections, 2, n_samples): every section gets the
 *                                       item's energy-type coefficients with N = S n_samples; the crest-factor delta lands on the one
 *                                       (section, sample) that holds the pooled peak; every section's mean-magnitude cotangent is the
 *                                       item's, formed from the pooled lin, with one more factor 1 / S; the adjoint transforms and the
 *                                       overlap-add then run per section as in every other backward
 * The analysis is that of the _items calls at bs = items * sections - the same launches and strip plan - followed by one pooling
 * launch; the workspace is mst_afloss_profile_workspace_bytes(items * sections, n_samples) for the loss and
 * mst_af_profile_workspace_bytes(items * sections, n_samples) for the profile (the pooled rows use a part of it that a one-set
 * analysis leaves unused).  sections = 1 gives the bits of the _items calls and of mst_af_profile; the loss of sections against their own
 * pooled profile is exactly 0 in all five terms; an item never reads another item's audio, profile row or cotangent.  Fixed-order
 * sums, no float atomics: bitwise reproducible; every buffer is written exactly up to its count.  items < 1, sections < 1,
 * n_samples <= 16384, a NULL pointer or a workspace that is too small return non-zero before anything is launched. */
int mst_af_profile_pooled(const float* x, int32_t items, int32_t sections, int64_t n_samples, const void* tables,
                          const float* filterbank, double* profile, void* workspace, size_t workspace_bytes, void* stream);
int mst_afloss_forward_profile_pooled(const float* pred, const double* profile, int32_t items, int32_t sections, int64_t n_samples,
                                      const float* weights5, const void* tables, const float* filterbank, float* losses, void* workspace,
                                      size_t workspace_bytes, void* stream);
int mst_afloss_backward_profile_pooled(const float* pred, const double* profile, int32_t items, int32_t sections, int64_t n_samples,
                                       const float* weights5, const void* tables, const float* filterbank, const float* grad_losses,
                                       float* grad_pred, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Spectrogram encoder: SpectrogramEncoder (reference mst/modules.py:740-806) = STFT front end +
 * Cnn14 (mst/panns.py:126-209, ConvBlock :27-85).  The 3x3 convolutions run on the matrix cores (MFMA); activations are
 * NHWC in the workspace; master weights, BatchNorm statistics and every gradient are fp32 in torch's own layouts.
 *
 * mst_spectrogram_forward: x (rows, n_samples) -> spec (rows, frames, bins) fp32 = (|STFT| + 1e-8)^0.3 with
 *   frames = 1 + n_samples / hop, bins = n_fft / 2 + 1 (torch.stft: periodic Hann, centre frames, reflect padding;
 *   modules.py:789-800).  n_fft = 2048 (the reference's the yaml files under configs/models).  Note the (frames, bins) order: the network
 *   below runs on the transposed image (its weights are transposed on the fly), nothing of it is user-visible. */
size_t mst_spectrogram_tables_bytes(void);
int mst_spectrogram_init_tables(void* tables, void* stream);
int mst_spectrogram_forward(const float* x, int32_t rows, int64_t n_samples, int32_t n_fft, int32_t hop, const void* tables,
                            float* spec, void* stream);

#define MST_CNN14_CONVS 12 /* six ConvBlocks x two convolutions, in forward order */
typedef struct mst_cnn14_desc {
    int32_t n;          /* signals = batch x channels of the encoder call */
    int32_t frames, bins;
    int32_t embed_dim;  /* num_classes of the final Linear(2048, embed_dim) */
    int32_t precision;  /* 0: bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16); 1: fp32 operands (v_mfma_f32_16x16x4_f32);
                         * 2: "bf16x3" - fp32 tensors everywhere (same buffers and sizes as 1), the convolutions' operands split into
                         *    bf16 (hi, lo) pairs on the way into the matrix pipe, x y ~ hi hi + hi lo + lo hi with fp32 accumulation
                         *    (~2^-17 per product); 3: "bf16x6" - the same with (hi, mid, lo) triples and the six product terms down to
                         *    2^-24: fp32-grade results (passes the parity bounds of precision 1) */
    int32_t training;   /* 1: BatchNorm2d with batch statistics (returned in batch_stats); 0: running statistics */
    float bn_eps;       /* 1e-5 */
    int32_t world;      /* 0 or 1: statistics over this call's signals.  > 1 (with a sync hook, mst_cnn14_forward_sync): BatchNorm statistics
                         * over `world` calls of equal n - torch.nn.SyncBatchNorm, reference configs/config.yaml:41 sync_batchnorm */
} mst_cnn14_desc;
typedef struct mst_cnn14_params { /* device pointers, fp32, torch layouts */
    const float* conv_w[MST_CNN14_CONVS];   /* (co, ci, 3, 3); channels 1-64-64-128-128-...-2048-2048 */
    const float* bn_gamma[MST_CNN14_CONVS]; /* BatchNorm2d weight */
    const float* bn_beta[MST_CNN14_CONVS];  /* BatchNorm2d bias */
    const float* bn_mean[MST_CNN14_CONVS];  /* running_mean (read when training = 0) */
    const float* bn_var[MST_CNN14_CONVS];   /* running_var */
    const float* fc_w;                      /* (embed_dim, 2048) */
    const float* fc_b;                      /* (embed_dim) */
} mst_cnn14_params;
typedef struct mst_cnn14_grads { /* device pointers, fp32, same layouts; every array is overwritten */
    float* conv_w[MST_CNN14_CONVS];
    float* bn_gamma[MST_CNN14_CONVS];
    float* bn_beta[MST_CNN14_CONVS];
    float* fc_w;
    float* fc_b;
} mst_cnn14_grads;
size_t mst_cnn14_workspace_bytes(const mst_cnn14_desc* d);
/* spec (n, frames, bins) fp32 -> embed (n, embed_dim).  batch_stats (12, 2, 2048) fp32 or NULL: per convolution the batch
 * mean and the biased batch variance of its output (training = 1) - what nn.BatchNorm2d folds into its running statistics.
 * The workspace keeps what mst_cnn14_backward needs. */
int mst_cnn14_forward(const mst_cnn14_desc* d, const float* spec, const mst_cnn14_params* params, float* embed,
                      float* batch_stats, void* workspace, size_t workspace_bytes, void* stream);
/* grad_embed (n, embed_dim) -> gradients of every parameter.  The spectrogram gets no gradient (the encoder's inputs are
 * audio, which the reference never differentiates: mst/system.py:284-300). */
int mst_cnn14_backward(const mst_cnn14_desc* d, const float* spec, const mst_cnn14_params* params, const float* grad_embed,
                       const mst_cnn14_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

/* Cross-rank BatchNorm statistics (reference: Lightning's sync_batchnorm = torch.nn.SyncBatchNorm over the process group,
 * configs/config.yaml:41, mst/panns.py:27-85).  The library has no communication of its own: between the per-channel fp64 sums of a
 * layer and their use it calls `sync(user, sums, n_doubles, stream)`, which must leave the ELEMENT-WISE SUM over all ranks in `sums`,
 * ordered after everything already queued on `stream` and before everything queued later (torch.distributed.all_reduce on a tensor that
 * aliases the workspace does exactly that).  Twelve calls per forward (sum, sum of squares of every convolution's output) and twelve
 * per backward (sum g, sum g xhat of every BatchNorm adjoint).  d->world = number of ranks (equal n on every rank).  The parameter
 * gradients of BatchNorm come out as (global sum) / world on every rank - what an averaging DistributedDataParallel leaves of the
 * per-rank sums.  sync == NULL or world <= 1 or training == 0: identical to mst_cnn14_forward / _backward. */
typedef void (*mst_sync_fn)(void* user, double* sums, size_t n_doubles, void* stream);
int mst_cnn14_forward_sync(const mst_cnn14_desc* d, const float* spec, const mst_cnn14_params* params, float* embed,
                           float* batch_stats, void* workspace, size_t workspace_bytes, void* stream, mst_sync_fn sync, void* user);
int mst_cnn14_backward_sync(const mst_cnn14_desc* d, const float* spec, const mst_cnn14_params* params, const float* grad_embed,
                            const mst_cnn14_grads* grads, void* workspace, size_t workspace_bytes, void* stream, mst_sync_fn sync,
                            void* user);

/* ---- One convolution of the encoder at a time (the seam of tests/test_conv_routes_gpu.py; DESIGN.md "The encoder's convolutions
 * per route").  Each entry runs, for one layer, exactly what mst_cnn14_forward / _backward run for it: the weight preparation, the
 * launcher (which chooses the kernel from the shape), and the fold of the partial results.  Images are NHWC in the transposed convention
 * of the network (h = frames, w = bins); weights and weight gradients are fp32 in torch's layout (cout, cin, 3, 3).  Activations are of
 * the storage type of `precision` (mst_cnn14_desc::precision): bf16 for 0, fp32 for 1 / 2 / 3.  cin and cout are powers of two in
 * 64 .. 2048, or cin = 1 with cout = 64 (the first layer: its input is the fp32 (n, h, w) spectrogram whatever the precision, and it
 * has no data gradient).  Every pointer is a device pointer aligned to 16 bytes, workspaces to 256. */
/* the two operand layouts of the prepared weights */
size_t mst_conv3x3_workspace_bytes(int32_t precision, int32_t cin, int32_t cout);
/* what the split-K route of this shape needs; 0: the shape is never split.  dgrad = 1: the data gradient (channel roles swapped) */
size_t mst_conv3x3_splitk_bytes(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dgrad);
/* room for the per-tile statistics of any route: (tiles, channels of the result, 2) fp32 with the smallest tile */
size_t mst_conv3x3_part_bytes(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t dgrad);
/* dgrad = 0: x (n, h, w, cin) -> out (n, h, w, cout); dgrad = 1: x is the cotangent (n, h, w, cout) -> out (n, h, w, cin).
 * part: NULL, or the per-tile sum / sum of squares of the fp32 results, (tiles, channels of out, 2); *tiles (host, may be NULL) gets
 * the tile count.  splitk: NULL (or too small) takes the unsplit route. */
int mst_conv3x3(int32_t precision, int32_t dgrad, const void* x, const float* weight, void* out, float* part, int32_t* tiles, int32_t n,
                int32_t h, int32_t w, int32_t cin, int32_t cout, void* workspace, size_t workspace_bytes, void* splitk, size_t splitk_bytes,
                void* stream);
/* the partial sums of the split the network chooses for this shape */
size_t mst_conv_wgrad_workspace_bytes(int32_t precision, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout);
/* dy (n, h, w, cout), x (n, h, w, cin) -> grad_weight (cout, cin, 3, 3) fp32, overwritten.  *splits / *steps_per_split (host, may be
 * NULL) get the pixel split that ran (steps of 32 pixels). */
int mst_conv_wgrad(int32_t precision, const void* dy, const void* x, float* grad_weight, int32_t n, int32_t h, int32_t w, int32_t cin,
                   int32_t cout, void* workspace, size_t workspace_bytes, int32_t* splits, int32_t* steps_per_split, void* stream);

/* ---- TransformerController encoder stack (reference mst/modules.py:848-854, :893-895: torch.nn.TransformerEncoder of
 * post-norm TransformerEncoderLayer(d_model, nhead, dim_feedforward, relu, dropout 0, batch_first) over the (bs, seq, d_model)
 * token sequence, with the key-padding mask of :880-890).  fp32 operands on v_mfma_f32_16x16x4_f32.  Limits: seq <= 128,
 * d_model % 128 == 0, d_model <= 1024, d_model / nhead <= 64, d_ff % 128 == 0, n_layers <= 16 (workspace_bytes returns 0 otherwise).
 * Stateless and re-entrant like the rest of the library; run-to-run deterministic (no atomics). */
typedef struct mst_ctrl_desc {
    int32_t bs, seq, d_model, nhead, d_ff, n_layers;
    float ln_eps; /* 1e-5 */
} mst_ctrl_desc;
typedef struct mst_ctrl_layer { /* device pointers, fp32, torch layouts (the state_dict entries of one layer) */
    const float* in_proj_weight;  /* self_attn.in_proj_weight (3 d_model, d_model) */
    const float* in_proj_bias;    /* (3 d_model) */
    const float* out_proj_weight; /* self_attn.out_proj.weight (d_model, d_model) */
    const float* out_proj_bias;
    const float* linear1_weight;  /* (d_ff, d_model) */
    const float* linear1_bias;
    const float* linear2_weight;  /* (d_model, d_ff) */
    const float* linear2_bias;
    const float* norm1_weight;
    const float* norm1_bias;
    const float* norm2_weight;
    const float* norm2_bias;
} mst_ctrl_layer;
typedef struct mst_ctrl_layer_grads { /* same entries; every array is overwritten */
    float* in_proj_weight;
    float* in_proj_bias;
    float* out_proj_weight;
    float* out_proj_bias;
    float* linear1_weight;
    float* linear1_bias;
    float* linear2_weight;
    float* linear2_bias;
    float* norm1_weight;
    float* norm1_bias;
    float* norm2_weight;
    float* norm2_bias;
} mst_ctrl_layer_grads;
size_t mst_ctrl_workspace_bytes(const mst_ctrl_desc* d);
/* tokens (bs, seq, d_model) -> out (bs, seq, d_model).  key_padding_mask (bs, seq) bytes, non-zero = ignore that key, or NULL.
 * layers: HOST array of n_layers entries.  The workspace keeps what mst_ctrl_backward needs. */
int mst_ctrl_forward(const mst_ctrl_desc* d, const float* tokens, const uint8_t* key_padding_mask, const mst_ctrl_layer* layers,
                     float* out, void* workspace, size_t workspace_bytes, void* stream);
/* grad_out (bs, seq, d_model) -> gradients of every layer parameter (grads: HOST array of n_layers entries) and of the tokens. */
int mst_ctrl_backward(const mst_ctrl_desc* d, const float* tokens, const mst_ctrl_layer* layers, const float* grad_out,
                      const mst_ctrl_layer_grads* grads, float* grad_tokens, void* workspace, size_t workspace_bytes, void* stream);

/* The controller's own ends (reference mst/modules.py:841-859, :866-914): the token sequence
 *   cat(track_embeds + track_embedding, mix_embeds + mix_embedding, fx_bus_embedding, master_bus_embedding)  (seq = n_tracks + 4)
 * with the key-padding mask extended by four always-attended tokens, and the three heads sigmoid(Linear) of the track tokens, the fx
 * token (seq - 2) and the master token (seq - 1).  n_t / n_f / n_m <= 32 outputs, d_model <= 1024.  A NULL head cotangent (g_f, g_m) means
 * that head's output was not used: its weight gradients are NOT written (the caller reports None, like autograd). */
typedef struct mst_ctrl_io { /* device pointers, fp32 */
    const float* track_embedding;      /* (d_model) */
    const float* mix_embedding;        /* (2, d_model) */
    const float* fx_bus_embedding;     /* (d_model) */
    const float* master_bus_embedding; /* (d_model) */
    const float* track_w;  const float* track_b;   /* track_projection (n_t, d_model), (n_t) */
    const float* fx_w;     const float* fx_b;
    const float* master_w; const float* master_b;
} mst_ctrl_io;
typedef struct mst_ctrl_io_grads { /* same entries; written by the two backward calls */
    float* track_embedding;
    float* mix_embedding;
    float* fx_bus_embedding;
    float* master_bus_embedding;
    float* track_w;  float* track_b;
    float* fx_w;     float* fx_b;
    float* master_w; float* master_b;
} mst_ctrl_io_grads;
int mst_ctrl_tokens_forward(const mst_ctrl_desc* d, int32_t n_tracks, const float* track_embeds, const float* mix_embeds,
                            const uint8_t* track_padding_mask, const mst_ctrl_io* io, float* tokens, uint8_t* key_padding_mask_out,
                            void* stream);
int mst_ctrl_heads_forward(const mst_ctrl_desc* d, int32_t n_tracks, const float* z, const mst_ctrl_io* io, int32_t n_t, int32_t n_f,
                           int32_t n_m, float* out_t, float* out_f, float* out_m, void* stream);
size_t mst_ctrl_heads_scratch_bytes(const mst_ctrl_desc* d, int32_t n_tracks);
/* grad_z (bs, seq, d_model): every row is written (the mix tokens get zeros); grads: the six head entries */
int mst_ctrl_heads_backward(const mst_ctrl_desc* d, int32_t n_tracks, const float* z, const mst_ctrl_io* io, int32_t n_t, int32_t n_f,
                            int32_t n_m, const float* out_t, const float* out_f, const float* out_m, const float* g_t, const float* g_f,
                            const float* g_m, const mst_ctrl_io_grads* grads, float* grad_z, void* scratch, void* stream);
/* grads: the four embedding entries; the cotangents of track_embeds / mix_embeds are the rows [0, T) / [T, T + 2) of grad_tokens */
int mst_ctrl_tokens_backward(const mst_ctrl_desc* d, int32_t n_tracks, const float* grad_tokens, const mst_ctrl_io_grads* grads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFMST_HIP_H */
