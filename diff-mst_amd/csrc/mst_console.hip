// mst_console.hip - C-ABI entry points of the mix console (include/diffmst_hip.h) and the
// launch sequences behind them.  No allocation, no host sync: everything is enqueued on the
// caller's stream over the caller's workspace.
#include "mst_kernels.h"
#include "mst_dev.h"

namespace mst {
static int check_desc(const mst_console_desc* d) {
    if (!d || d->bs <= 0 || d->n_tracks <= 0 || d->n_samples <= 0) return hipErrorInvalidValue;
    if (d->flags & MST_USE_FX_BUS) {
        if (d->fx_ir_samples < 4096 || d->fx_ir_samples % 4096 || d->fx_ir_samples > (1 << 20)) return hipErrorInvalidValue;
        if (d->fx_bandpass_taps < 1 || d->fx_bandpass_taps > 1023 || !(d->fx_bandpass_taps & 1)) return hipErrorInvalidValue;
    }
    if (!(d->flags & MST_USE_TRACK_PANNER)) return hipErrorInvalidValue;  // reference branch is broken (mst/modules.py:269)
    if (d->track_row_stride < d->n_samples) return hipErrorInvalidValue;
    if ((d->track_lookahead & 3) || (d->master_lookahead & 3) || d->track_lookahead < 0 || d->master_lookahead < 0)
        return hipErrorInvalidValue;
    return hipSuccess;
}
}  // namespace mst

using namespace mst;

extern "C" int mst_abi_version(void) { return 13; }
MST_DEV_PROBE_STATE  // developer probe, mst_dev.h (nothing in a default build)

extern "C" size_t mst_console_fx_tables_bytes(void) { return (size_t)8192 * 2 * sizeof(float); }
extern "C" int mst_console_fx_init_tables(void* tables, void* stream) {
    if (!tables) return hipErrorInvalidValue;
    launch_fx_tables((float*)tables, (hipStream_t)stream);
    return (int)hipGetLastError();
}

static FxPlan fx_plan(const Layout& L) {
    FxPlan p{};
    p.bs = L.bs;
    p.S = L.fxS;
    p.taps = L.fxTaps;
    p.K = L.fxK;
    p.nblk = L.fxBlk;
    p.nblk_ir = L.fxBlkIr;
    p.n = L.N;
    p.Ns = row_stride(L.N);
    p.rcfx = L.fx_rc; p.fx_in = L.fx_in; p.wnf = L.fx_wnf; p.ir = L.fx_ir; p.Xs = L.fx_Xs; p.Hs = L.fx_Hs; p.Ys = L.fx_Ys;
    p.dXs = L.fx_dXs; p.dHs = L.fx_dHs; p.dir = L.fx_dir; p.dfx_in = L.fx_din; p.fxpart = L.fx_part; p.Hf = L.fx_Hf; p.mixv = L.fx_mix; p.dry = L.fx_dry;
    return p;
}

// MST_SPLIT_BATCH (ABI v9): the mixes of a call are dealt to two halves that run as two independent console calls - the first on the
// caller's stream, the second on a side stream the caller lends (mst_console_overlap) - each over its own part of the workspace.  The
// two halves' launches interleave on the device: the first half's latency-bound stretches (k_prep's fp64 chains, the lone-wave master
// chain, the single-workgroup tails) run beside the second half's occupancy-full track kernels and vice versa.  Same kernels, same
// arithmetic per mix: results are bit-identical to the unsplit call.
static bool split_on(const mst_console_desc* d) {
    return (d->flags & MST_SPLIT_BATCH) && d->bs >= 2 && !(d->flags & MST_USE_FX_BUS) && !basic_path(d);
}
struct Halves {
    mst_console_desc da, db;
    int64_t ws_b;  // float offset of the second half's workspace
    int64_t total;
};
static Halves make_halves(const mst_console_desc* d) {
    Halves h{*d, *d, 0, 0};
    h.da.bs = d->bs / 2;
    h.db.bs = d->bs - h.da.bs;
    h.da.flags &= ~MST_SPLIT_BATCH;
    h.db.flags &= ~MST_SPLIT_BATCH;
    h.ws_b = make_layout(&h.da).total;
    h.total = h.ws_b + make_layout(&h.db).total;
    return h;
}
static bool overlap_ok(const mst_console_overlap* ov) { return ov && ov->side_stream && ov->fork_event && ov->join_event; }
// the caller's workspace: there, large enough, 256-byte aligned (every array inside is laid out on 256 bytes)
static bool workspace_ok(const void* workspace, size_t workspace_bytes, int64_t floats) {
    return workspace && workspace_bytes >= (size_t)floats * sizeof(float) && !((uintptr_t)workspace & 255);
}
// Fork, both halves, join.  half(desc, b0, workspace, bytes, stream) enqueues the console call of the mixes from b0 on.
template <class Half>
static int split_call(const mst_console_desc* d, void* workspace, size_t workspace_bytes, void* stream, const mst_console_overlap* ov, Half half) {
    if (!overlap_ok(ov) || ov->side_stream == stream) return hipErrorInvalidValue;
    const Halves h = make_halves(d);
    if (!workspace_ok(workspace, workspace_bytes, h.total)) return hipErrorInvalidValue;
    hipStream_t main_s = (hipStream_t)stream, side = (hipStream_t)ov->side_stream;
    if (int e = (int)hipEventRecord((hipEvent_t)ov->fork_event, main_s)) return e;
    if (int e = (int)hipStreamWaitEvent(side, (hipEvent_t)ov->fork_event, 0)) return e;
    float* ws = (float*)workspace;
    // the second half first: its stream has just been released and its k_prep is the first thing the device can start beside the main stream's
    int e = half(&h.db, (int64_t)h.da.bs, ws + h.ws_b, (size_t)(h.total - h.ws_b) * sizeof(float), side);
    if (!e) e = half(&h.da, (int64_t)0, ws, (size_t)h.ws_b * sizeof(float), main_s);
    // always rejoin (also after an error: a captured graph must not end with the side stream forked)
    (void)hipEventRecord((hipEvent_t)ov->join_event, side);
    (void)hipStreamWaitEvent(main_s, (hipEvent_t)ov->join_event, 0);
    return e ? e : (int)hipGetLastError();
}
// p advanced to mix b0 of an array with `per_mix` elements per mix; null stays null
template <class T>
static T* from_mix(T* p, int64_t b0, int64_t per_mix) { return p ? p + b0 * per_mix : nullptr; }

extern "C" size_t mst_console_workspace_bytes(const mst_console_desc* d) {
    if (check_desc(d) != hipSuccess) return 0;
    if (split_on(d)) return (size_t)make_halves(d).total * sizeof(float);
    return (size_t)make_layout(d).total * sizeof(float);
}

static BasicArgs basic_args(const mst_console_desc* d, const float* tracks, const float* track_params, const float* fx_bus_params,
                            const float* master_bus_params, float* part) {
    BasicArgs ba{};
    ba.tracks = tracks;
    ba.track_params = track_params;
    ba.fx_params = fx_bus_params;
    ba.master_params = master_bus_params;
    ba.part = part;
    ba.d = *d;
    return ba;
}
// the verdict of the range check, mirrored to the host (mst_console_forward_mirrored)
static void mirror_status(const int32_t* status, int32_t* status_host, void* status_event, hipStream_t stream) {
    if (!status_host) return;
    (void)hipMemcpyAsync(status_host, status, sizeof(int32_t), hipMemcpyDeviceToHost, stream);
    if (status_event) (void)hipEventRecord((hipEvent_t)status_event, stream);
}

static int console_forward_impl(const mst_console_desc* d, const float* tracks, const float* track_params,
                                const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                void* stream_, int32_t* status_host, void* status_event) {
    if (int e = check_desc(d)) return e;
    const Layout L = make_layout(d);
    if (!workspace_ok(workspace, workspace_bytes, L.total)) return hipErrorInvalidValue;
    if (!tracks || !track_params || !fx_bus_params || !master_bus_params || !mix || !status) return hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    float* ws = (float*)workspace;
    const int64_t n = L.N, Ns = row_stride(L.N);
    const bool save = d->flags & MST_SAVE_FOR_BACKWARD;
    const int aligned = (n % 4 == 0) && !((uintptr_t)mix & 15) && !((uintptr_t)mixed_tracks & 15);
    const bool t_comp = d->flags & MST_USE_TRACK_COMPRESSOR;
    const bool m_on = d->flags & MST_USE_MASTER_BUS;
    const bool o_on = d->flags & MST_USE_OUTPUT_FADER;
    const bool fx_on = d->flags & MST_USE_FX_BUS;
    if (fx_on && (!fx || !fx->noise || !fx->filters || !fx->tables)) return hipErrorInvalidValue;
    if (basic_path(d)) {  // BASELINE cfg #1: gain + pan + bus sum in one launch
        BasicArgs ba = basic_args(d, tracks, track_params, fx_bus_params, master_bus_params, ws + L.cp_t);
        ba.mix = mix;
        ba.mixed = mixed_tracks;
        ba.status = status;
        launch_basic_forward(ba, stream);
        mirror_status(status, status_host, status_event, stream);
        return (int)hipGetLastError();
    }
    // The backward's coefficient-gradient walk reads the all-pole chunk start states over the PADDED chunk count and multiplies the
    // padding by samples that are exactly zero; no launch writes that padding and the workspace comes as the caller allocated it, so
    // a NaN left there would come out as a NaN gradient.  Only lengths whose chunk count is no multiple of 256 have any.
    if (save && L.ncE_pad != L.ncE)
        (void)hipMemsetAsync(ws + L.sP_t, 0, (size_t)(L.R + 2 * L.bs) * 24 * L.ncE_pad * sizeof(float), stream);

    // ---- prep: row constants, scan tables and zero-state maps of every EQ pass of the call (both directions), granules zeroed
    EqPass eq_t = eq_rows(L, ws, EQ_TRACKS, EQ_FWD), eq_m = eq_rows(L, ws, EQ_MASTER, EQ_FWD);
    const EqPass adj_t = eq_rows(L, ws, EQ_TRACKS, EQ_ADJ), adj_m = eq_rows(L, ws, EQ_MASTER, EQ_ADJ);
    const ApScanJobs ap_t = allpole_rows(L, ws, EQ_TRACKS), ap_m = allpole_rows(L, ws, EQ_MASTER);
    PrepArgs pa{};
    pa.track_params = track_params;
    pa.fx_params = fx_bus_params;
    pa.master_params = master_bus_params;
    pa.rc_t = ws + L.rc_t; pa.rc_m = ws + L.rc_m;
    pa.powF_t = eq_t.pow; pa.powF_m = eq_m.pow;
    pa.powA_t = adj_t.pow; pa.powA_m = adj_m.pow;
    pa.powP_t = ap_t.tab; pa.powP_m = ap_m.tab;
    pa.pow1F_t = eq_t.pow1; pa.pow1F_m = eq_m.pow1;
    pa.pow1A_t = adj_t.pow1; pa.pow1A_m = adj_m.pow1;
    pa.wzF_t = eq_t.wz; pa.wzF_m = eq_m.wz;
    pa.wzA_t = adj_t.wz; pa.wzA_m = adj_m.wz;
    if (fx_on) {
        pa.rc_fx = ws + L.fx_rc;
        pa.fx_mix = ws + L.fx_mix;
    }
    pa.status = status;
    pa.R = L.R; pa.bs = L.bs;
    pa.KE = L.KE;
    pa.eq1 = L.eq1;
    pa.d = *d;
    pa.gran = (gran_t*)(ws + L.gran_f);
    pa.gran_n = L.gran_nf + L.gran_nb;
#ifndef MST_PREP_RIDER_MAX_BYTES
#define MST_PREP_RIDER_MAX_BYTES (128ll << 20)  // the riders pull the track rows through the 256 MB Infinity Cache for the launch that follows:
                                                // only while the rows fit it (cfg #2: 67 MB).  At cfg #3 (537 MB) they were 120 us of k_prep
                                                // for rows that were gone again before the EQ pass read them
#endif
    if (n % 4 == 0 && d->track_row_stride % 4 == 0 && !((uintptr_t)tracks & 15) && (int64_t)L.R * n * 4 <= MST_PREP_RIDER_MAX_BYTES) {
        pa.pf_src = tracks;
        pa.pf_stride = d->track_row_stride;
        pa.pf_n = n;
    }
    launch_prep(pa, stream);
    // the range check is complete when k_prep is: its verdict travels to the host NOW, behind k_prep and ahead of the rest of the forward
    // (mst_console_forward_mirrored) - a caller that wants the reference's immediate ValueError waits for this copy, not for the mix
    mirror_status(status, status_host, status_event, stream);
    MST_DEV_PROBE_AT(0, stream);

    // ---- tracks: EQ (+ the gain computer and the compressor smoother's block aggregates), apply + pan + bus sum
    eq_t.in = tracks;
    eq_t.in_stride = d->track_row_stride;
    eq_t.status = status;
    if (t_comp) {
        eq_t.zs_comp = ws + L.zS_t;
        eq_t.nblk_comp = L.nblkC;
    }
    // a call that saves for backward also leaves the all-pole zero-state ends of the coefficient-gradient pass
    if (save) eq_t.zp = ap_t.z;
    launch_eq_pass(eq_t, stream);
    const bool bus_is_mix = !m_on && !o_on;
    float* busp = bus_is_mix ? mix : ws + L.bus;
    const int64_t bus_stride = bus_is_mix ? n : Ns;
    TrackApplyArgs ta{};
    ta.u = eq_t.out;
    ta.stride = Ns;
    ta.rc = eq_t.rc;
    ta.s0 = ws + L.zS_t;
    if (save && t_comp) ta.gs = ws + L.gs_t;
    ta.bus = busp;
    ta.bus_stride = bus_stride;
    ta.mixed = mixed_tracks;
    if (fx_on) ta.fx = ws + L.fx_in;
    ta.T = L.T; ta.nc_pad = L.ncC_pad; ta.lookahead = d->track_lookahead; ta.comp_on = t_comp ? 1 : 0;
    ta.n = n;
    ta.aligned = aligned;
    launch_apply_tracks(ta, L.bs, stream);
    MST_DEV_PROBE_AT(1, stream);
    // ---- fx bus: reverberate the send bus and add it to the stereo bus (reference mst/modules.py:275-284)
    if (fx_on) launch_fx_forward(fx_plan(L), fx->noise, fx->filters, (const float*)fx->tables, ws, busp, bus_stride, stream);

    // ---- master bus: EQ, compressor + output fader -> mix
    MasterApplyArgs ma{};
    ma.stride = Ns;
    ma.rc = eq_m.rc;
    ma.out = mix;
    ma.out_stride = n;
    ma.nc_pad = L.ncC_pad;
    ma.n = n;
    ma.aligned = aligned;
    if (m_on) {
        eq_m.status = status;
        if (save) eq_m.zp = ap_m.z;
        // + the track rows' all-pole carry scan as extra workgroups of the (one wave per SIMD) run launch
        if (L.apscan_fwd && eq_m.zp && eq_t.zp && eq_m.eq1) eq_m.scan = ap_t;
        launch_eq_pass(eq_m, stream);
        ma.v = eq_m.out;
        ma.s0 = ws + L.zS_m;
        if (save) ma.gs = ws + L.gs_m;
        ma.lookahead = d->master_lookahead; ma.comp_on = 1;
        ma.gran = (gran_t*)(ws + L.gran_f);
        ma.gran_near = (int64_t)L.bs * L.nblkC;
        ma.status = status;
        launch_apply_master(ma, L.bs, stream);
    } else if (o_on) {  // output fader only
        ma.v = ws + L.bus;
        launch_apply_master(ma, L.bs, stream);
    }
    return (int)hipGetLastError();
}

extern "C" int mst_console_forward(const mst_console_desc* d, const float* tracks, const float* track_params,
                                   const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                   float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (d && (d->flags & MST_SPLIT_BATCH)) return hipErrorInvalidValue;  // the split form needs the side stream: mst_console_forward_overlapped
    return console_forward_impl(d, tracks, track_params, fx_bus_params, master_bus_params, fx, mix, mixed_tracks, status, workspace,
                                workspace_bytes, stream, nullptr, nullptr);
}
extern "C" int mst_console_forward_overlapped(const mst_console_desc* d, const float* tracks, const float* track_params,
                                              const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                              float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                              void* stream, const mst_console_overlap* ov) {
    if (int e = check_desc(d)) return e;
    if (!split_on(d))
        return console_forward_impl(d, tracks, track_params, fx_bus_params, master_bus_params, fx, mix, mixed_tracks, status, workspace,
                                    workspace_bytes, stream, nullptr, nullptr);
    if (!tracks || !track_params || !fx_bus_params || !master_bus_params || !mix || !status) return hipErrorInvalidValue;
    const int64_t T = d->n_tracks, n = d->n_samples;
    return split_call(d, workspace, workspace_bytes, stream, ov, [&](const mst_console_desc* dh, int64_t b0, float* ws, size_t ws_bytes, hipStream_t s) {
        return console_forward_impl(dh, tracks + b0 * T * d->track_row_stride, track_params + b0 * T * MST_NUM_TRACK_PARAMS,
                                    fx_bus_params + b0 * MST_NUM_FX_PARAMS, master_bus_params + b0 * MST_NUM_MASTER_PARAMS, nullptr, mix + b0 * 2 * n,
                                    from_mix(mixed_tracks, b0, 2 * T * n), status, ws, ws_bytes, s, nullptr, nullptr);
    });
}
extern "C" int mst_console_forward_mirrored(const mst_console_desc* d, const float* tracks, const float* track_params,
                                            const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                            float* mix, float* mixed_tracks, int32_t* status, void* workspace, size_t workspace_bytes,
                                            void* stream, int32_t* status_host, void* status_event) {
    if (!status || !status_host) return hipErrorInvalidValue;
    if (d && (d->flags & MST_SPLIT_BATCH)) return hipErrorInvalidValue;  // the mirrored verdict is formed by ONE k_prep: no split form
    return console_forward_impl(d, tracks, track_params, fx_bus_params, master_bus_params, fx, mix, mixed_tracks, status, workspace,
                                workspace_bytes, stream, status_host, status_event);
}

// carry scan of the all-pole bank's chunk states: every row, or - when the forward's master-bus run already carried the track rows'
// (Layout::apscan_fwd) - nothing up front: the master rows' ride on the backward's adjoint run
static void allpole_scan(const Layout& L, float* ws, int nsig_all, hipStream_t stream) {
    const ApScanJobs ap = allpole_rows(L, ws, EQ_TRACKS);  // the master rows follow the track rows in the same arrays
    if (!L.apscan_fwd) launch_scan2(ap.z, ap.s0, ap.tab, L.R, L.ncE, L.ncE_pad, L.KE, nsig_all, stream);
}

extern "C" int mst_console_backward_prepare(const mst_console_desc* d, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int e = check_desc(d)) return e;
    const Layout L = make_layout(d);
    if (!workspace_ok(workspace, workspace_bytes, L.total)) return hipErrorInvalidValue;
    if (!(d->flags & MST_SAVE_FOR_BACKWARD) || (d->flags & MST_SPLIT_BATCH)) return hipErrorInvalidValue;
    float* ws = (float*)workspace;
    const int nsig_all = L.R + ((d->flags & MST_USE_MASTER_BUS) ? 2 * L.bs : 0);
    allpole_scan(L, ws, nsig_all, (hipStream_t)stream_);
    return (int)hipGetLastError();
}

static int console_backward_impl(const mst_console_desc* d, const float* tracks, const float* track_params,
                                 const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                 const float* grad_mix, const float* grad_mixed_tracks, float* grad_track_params,
                                 float* grad_fx_params, float* grad_master_params, float* grad_tracks, int32_t* status,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
    if (int e = check_desc(d)) return e;
    const Layout L = make_layout(d);
    if (!workspace_ok(workspace, workspace_bytes, L.total)) return hipErrorInvalidValue;
    if (!(d->flags & MST_SAVE_FOR_BACKWARD)) return hipErrorInvalidValue;
    if (!track_params || !master_bus_params || !grad_mix || !grad_track_params || !grad_master_params) return hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    float* ws = (float*)workspace;
    const int64_t n = L.N, Ns = row_stride(L.N);
    const bool t_comp = d->flags & MST_USE_TRACK_COMPRESSOR;
    const bool m_on = d->flags & MST_USE_MASTER_BUS;
    const bool o_on = d->flags & MST_USE_OUTPUT_FADER;
    const bool fx_on = d->flags & MST_USE_FX_BUS;
    if (fx_on && (!fx || !fx->tables || !fx_bus_params)) return hipErrorInvalidValue;
    const int aligned = (n % 4 == 0) && !((uintptr_t)grad_mix & 15) && !((uintptr_t)grad_mixed_tracks & 15);
    if (basic_path(d)) {
        if (!tracks) return hipErrorInvalidValue;
        BasicArgs ba = basic_args(d, tracks, track_params, fx_bus_params, master_bus_params, ws + L.cp_t);
        ba.grad_mix = grad_mix;
        ba.grad_mixed = grad_mixed_tracks;
        ba.grad_track_params = grad_track_params;
        ba.grad_master_params = grad_master_params;
        ba.grad_tracks = grad_tracks;
        launch_basic_backward(ba, stream);
        return (int)hipGetLastError();
    }

    // ---- all-pole states of the coefficient-gradient pass depend only on what forward saved: one
    // launch covers the track rows and the master rows (signal rows [0,R) and [R,R+2bs) of the same arrays)
    const int nsig_all = L.R + (m_on ? 2 * L.bs : 0);
    if (!(d->flags & MST_BWD_PREPARED)) {  // else: mst_console_backward_prepare ran (on a side stream the caller has joined)
        allpole_scan(L, ws, nsig_all, stream);
    }
    const ApScanJobs ap_t = allpole_rows(L, ws, EQ_TRACKS), ap_m = allpole_rows(L, ws, EQ_MASTER);
    EqPass adj_m = eq_rows(L, ws, EQ_MASTER, EQ_ADJ), adj_t = eq_rows(L, ws, EQ_TRACKS, EQ_ADJ);
    // coefficient-gradient sums of the two channels of every master bus: in the master launch (round 3), or - when the all-pole scans ride
    // on other launches (Layout::apscan_fwd) - as extra rows of the TRACKS' run launch below: the master launch is one lockstep round of lone
    // workgroups, where two more 64-sample walks per workgroup are pure latency (31 -> 18 us), the track launch absorbs them
    const bool master_cg_later = L.apscan_fwd;

    // ---- master bus: compressor + output fader adjoint, EQ adjoint (-> grad of the stereo bus)
    const float* gbus = grad_mix;  // cotangent of the stereo bus as seen by the track stage
    int64_t gbus_stride = n;
    if (m_on || o_on) {
        CompBwdArgs ca{};
        ca.stride = Ns;
        ca.rc = adj_m.rc;
        ca.part = ws + L.cp_m;
        ca.gup = grad_mix;
        ca.gup_stride = n;
        ca.T = 1; ca.nc_pad = L.ncC_pad;
        ca.n = n;
        ca.aligned = aligned;
        if (m_on) {
            ca.u = ws + L.v_m;
            ca.gs = ws + L.gs_m;
            ca.zq = ws + L.zQ_m;
            ca.du = ws + L.du_m;
            ca.lookahead = d->master_lookahead; ca.comp_on = 1;
            // the adjoint smoother's block aggregates are exchanged inside the run launch (mst_common.h: granules)
            ca.gran = (gran_t*)(ws + L.gran_b) + 2 * (int64_t)L.R * L.nblkC;
            ca.gran_near = (int64_t)L.bs * L.nblkC;
            ca.status = status;
            ca.s0 = ws + L.zQ_m;
            if (!master_cg_later) {
                ca.ap_s0 = ap_m.s0;
                ca.ap_nc_pad = L.ncE_pad;
                ca.ep = ws + L.ep_m;
            }
            launch_comp_bwd(true, ca, L.bs, stream);
            adj_m.status = status;
            // + the master rows' own all-pole carry scans as extra workgroups of the (one wave per SIMD) run launch
            if (master_cg_later) adj_m.scan = ap_m;
            launch_eq_pass(adj_m, stream);
        } else {  // output fader only
            ca.u = ws + L.bus;
            ca.du = ws + L.dbus;
            launch_comp_bwd(true, ca, L.bs, stream);
        }
        gbus = ws + L.dbus;
        gbus_stride = Ns;
    } else {
        (void)hipMemsetAsync(ws + L.cp_m, 0, (size_t)L.bs * L.nblkC * CP_COUNT * sizeof(float), stream);
    }

    // ---- fx bus: the wet signal was added to the stereo bus, so its cotangent is the bus cotangent
    if (fx_on) launch_fx_backward(fx_plan(L), gbus, gbus_stride, (const float*)fx->tables, ws, stream);

    // ---- tracks: pan + compressor adjoint, EQ adjoint (-> grad_tracks)
    CompBwdArgs ca{};
    ca.u = ws + L.u_t;
    ca.stride = Ns;
    ca.gs = ws + L.gs_t;
    ca.rc = adj_t.rc;
    ca.zq = ws + L.zQ_t;
    ca.du = ws + L.du_t;
    ca.part = ws + L.cp_t;
    ca.gup = gbus;
    ca.gup_stride = gbus_stride;
    ca.gmixed = grad_mixed_tracks;
    if (fx_on) ca.gfx = ws + L.fx_din;
    ca.gfx_stride = Ns;
    ca.T = L.T; ca.nc_pad = L.ncC_pad; ca.lookahead = d->track_lookahead; ca.comp_on = t_comp ? 1 : 0;
    ca.n = n;
    ca.aligned = aligned;
    if (t_comp) {
        ca.gran = (gran_t*)(ws + L.gran_b);
        ca.gran_near = (int64_t)L.R * L.nblkC;
        ca.status = status;
        ca.s0 = ws + L.zQ_t;
    }
    // the run pass forms the tracks' coefficient-gradient sums from the du and u it holds in registers: du crosses HBM only
    // when the EQ adjoint below needs it (grad_tracks), u is not read a second time
    ca.ap_s0 = ap_t.s0;
    ca.ap_nc_pad = L.ncE_pad;
    ca.ep = ws + L.ep_t;
    if (!grad_tracks) ca.du = nullptr;
    if (m_on && master_cg_later) {  // the master channels' coefficient-gradient walks ride here (see above)
        ca.cg2_u = ws + L.v_m;
        ca.cg2_du = ws + L.du_m;
        ca.cg2_rc = adj_m.rc;
        ca.cg2_rows = 2 * L.bs;
    }
    launch_comp_bwd(false, ca, L.R, stream);
    if (grad_tracks) {
        adj_t.out = grad_tracks;
        adj_t.out_stride = n;
        launch_eq_pass(adj_t, stream);
    }

    // ---- prep: partial sums -> parameter gradients, the backward's granules re-armed
    PrepBwdArgs pb{};
    pb.track_params = track_params;
    pb.master_params = master_bus_params;
    pb.rc_t = adj_t.rc; pb.rc_m = adj_m.rc;
    pb.cp_t = ws + L.cp_t; pb.cp_m = ws + L.cp_m;
    pb.ep_t = ws + L.ep_t; pb.ep_m = ws + L.ep_m;
    pb.grad_track_params = grad_track_params;
    pb.grad_master_params = grad_master_params;
    pb.fx_params = fx_bus_params;
    pb.nblkF = L.fxBlkIr;
    pb.nblkX = L.fxBlk;
    if (fx_on) {
        pb.fx_part = ws + L.fx_part;
        pb.grad_fx_params = grad_fx_params;
        pb.fx_mix = ws + L.fx_mix;
        pb.fx_dry = ws + L.fx_dry;
    }
    pb.R = L.R; pb.bs = L.bs; pb.nblkC = L.nblkC; pb.nblkE = L.nblkE;
    pb.nblkEt = L.nblkEt;
    pb.d = *d;
    pb.gran = (gran_t*)(ws + L.gran_b);
    pb.gran_n = L.gran_nb;
    launch_prep_bwd(pb, stream);
    return (int)hipGetLastError();
}

extern "C" int mst_console_backward(const mst_console_desc* d, const float* tracks, const float* track_params,
                                    const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                    const float* grad_mix, const float* grad_mixed_tracks, float* grad_track_params,
                                    float* grad_fx_params, float* grad_master_params, float* grad_tracks, int32_t* status,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (d && (d->flags & MST_SPLIT_BATCH)) return hipErrorInvalidValue;  // mst_console_backward_overlapped
    return console_backward_impl(d, tracks, track_params, fx_bus_params, master_bus_params, fx, grad_mix, grad_mixed_tracks, grad_track_params,
                                 grad_fx_params, grad_master_params, grad_tracks, status, workspace, workspace_bytes, stream);
}
extern "C" int mst_console_backward_overlapped(const mst_console_desc* d, const float* tracks, const float* track_params,
                                               const float* fx_bus_params, const float* master_bus_params, const mst_console_fx* fx,
                                               const float* grad_mix, const float* grad_mixed_tracks, float* grad_track_params,
                                               float* grad_fx_params, float* grad_master_params, float* grad_tracks, int32_t* status,
                                               void* workspace, size_t workspace_bytes, void* stream, const mst_console_overlap* ov) {
    if (int e = check_desc(d)) return e;
    if (!split_on(d))
        return console_backward_impl(d, tracks, track_params, fx_bus_params, master_bus_params, fx, grad_mix, grad_mixed_tracks, grad_track_params,
                                     grad_fx_params, grad_master_params, grad_tracks, status, workspace, workspace_bytes, stream);
    if (d->flags & MST_BWD_PREPARED) return hipErrorInvalidValue;
    if (!track_params || !master_bus_params || !grad_mix || !grad_track_params || !grad_master_params) return hipErrorInvalidValue;
    const int64_t T = d->n_tracks, n = d->n_samples;
    return split_call(d, workspace, workspace_bytes, stream, ov, [&](const mst_console_desc* dh, int64_t b0, float* ws, size_t ws_bytes, hipStream_t s) {
        return console_backward_impl(dh, from_mix(tracks, b0, T * d->track_row_stride), track_params + b0 * T * MST_NUM_TRACK_PARAMS,
                                     from_mix(fx_bus_params, b0, MST_NUM_FX_PARAMS), master_bus_params + b0 * MST_NUM_MASTER_PARAMS, nullptr,
                                     grad_mix + b0 * 2 * n, from_mix(grad_mixed_tracks, b0, 2 * T * n), grad_track_params + b0 * T * MST_NUM_TRACK_PARAMS,
                                     nullptr, grad_master_params + b0 * MST_NUM_MASTER_PARAMS, from_mix(grad_tracks, b0, T * n), status, ws, ws_bytes, s);
    });
}
