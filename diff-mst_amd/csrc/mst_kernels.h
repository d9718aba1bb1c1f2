// mst_kernels.h - what the console translation units share on the host side (each kernel is launched only from the file that
// defines it: no relocatable device code):
//   - the kernels' argument blocks (PrepArgs ... CompBwdArgs), passed by value and filled BY MEMBER NAME wherever they are built;
//   - EqPass, the description of one EQ pass over one family of rows, eq_rows() / allpole_rows(), the views of the workspace layout
//     that fill it, and launch_eq_pass(), which turns it into launches;
//   - the launch functions of the other stages.
#pragma once
#include "mst_common.h"

namespace mst {

enum { EQ_FWD = 0, EQ_ADJ = 1 };
// `split` arguments: signal rows below it are mono (tracks, one filter row each), rows from it on are stereo
// pairs sharing a filter row (master buses).  Tracks-only launch: split = nsig; master-only: split = 0.

// ---- mst_params.hip
struct PrepArgs {
    const float* track_params;   // (R, 27)
    const float* fx_params;      // (bs, 25)
    const float* master_params;  // (bs, 26)
    float* rc_t;
    float* rc_m;
    float* powF_t; float* powF_m;  // forward-cascade scan tables
    float* powA_t; float* powA_m;  // adjoint-cascade scan tables
    float* powP_t; float* powP_m;  // all-pole scan tables
    float* pow1F_t; float* pow1F_m;  // in-wave scan tables (forward / adjoint cascade)
    float* pow1A_t; float* pow1A_m;
    float* wzF_t; float* wzF_m;      // zero-state maps of the forward / adjoint cascade (eq1 only)
    float* wzA_t; float* wzA_m;
    float* rc_fx;   // (bs, 24): reverberation band gains (times the wet/dry mix) and decay rates 10 d + 1 (fx bus), or nullptr
    float* fx_mix;  // (bs): wet/dry mix - 1 (reference mst/modules.py:420) unless MST_NO_RANGE_CHECK hands a value over
    int32_t* status;
    int R, bs;
    int KE;  // chunks per scan lane (EQ scans)
    int eq1; // which family of cascade tables to build (Layout::eq1)
    mst_console_desc d;
    gran_t* gran;       // every granule array of the call (mst_common.h), zeroed here
    int64_t gran_n;
    // prefetch riders (mst_params.hip: k_prep): R rows of pf_n floats, pf_stride apart, pulled through the Infinity Cache while the
    // design chains run; null = none.  Rows must be 16-byte aligned with pf_n % 4 == 0.
    const float* pf_src;
    int64_t pf_stride, pf_n;
};
struct PrepBwdArgs {
    const float* track_params;
    const float* master_params;
    const float* rc_t;
    const float* rc_m;
    const float* cp_t; const float* cp_m;  // compressor partial sums  rows x nblkC x CP_COUNT
    const float* ep_t; const float* ep_m;  // coefficient partial sums sigrows x nblkE x EP_COUNT
    float* grad_track_params;              // (R,27)
    float* grad_master_params;             // (bs,26)
    const float* fx_params;                // (bs,25) fx bus only
    const float* fx_part;                  // (bs, nblkF, 24) partial sums of the reverberation parameters, or nullptr
    float* grad_fx_params;                 // (bs,25) or nullptr
    int nblkF;
    const float* fx_mix;                   // (bs) wet/dry mix used by forward
    const float* fx_dry;                   // (bs, nblkX) partial sums <dbus, fx_in>
    int nblkX;
    int R, bs, nblkC, nblkE;
    int nblkEt;                            // partial rows per track row (Layout::nblkEt)
    mst_console_desc d;
    gran_t* gran;                          // the backward's granule arrays, re-armed (zeroed) for a second backward over the same forward
    int64_t gran_n;
};
// BASELINE cfg #1 (gain + pan + bus sum only): one forward launch, two backward launches, no k_prep chain (mst_params.hip)
constexpr int kBasicMaxTracks = 256;
struct BasicArgs {
    const float* tracks;         // (bs, T, n), row stride d.track_row_stride
    const float* track_params;   // (bs, T, 27)
    const float* fx_params;      // (bs, 25)   range check only
    const float* master_params;  // (bs, 26)   range check only
    float* mix;                  // (bs, 2, n) forward out
    float* mixed;                // (bs, 2, T, n) forward out or null
    int32_t* status;
    const float* grad_mix;       // backward in
    const float* grad_mixed;     // (bs, 2, T, n) or null
    float* grad_track_params;    // (bs, T, 27) out
    float* grad_master_params;   // (bs, 26) out (zeros) or null
    float* grad_tracks;          // (bs, T, n) out or null
    float* part;                 // (bs, nblk, T, 2) scratch
    mst_console_desc d;
};
inline bool basic_path(const mst_console_desc* d) {  // every stage but input fader / panner off, and few enough tracks for the LDS table
    const uint32_t stages = MST_USE_TRACK_EQ | MST_USE_TRACK_COMPRESSOR | MST_USE_FX_BUS | MST_USE_MASTER_BUS | MST_USE_OUTPUT_FADER;
    return !(d->flags & stages) && (d->flags & MST_USE_TRACK_PANNER) && d->n_tracks <= kBasicMaxTracks && !(d->flags & MST_DEV_MULTIPASS_EQ);
}
void launch_basic_forward(const BasicArgs& a, hipStream_t stream);
void launch_basic_backward(const BasicArgs& a, hipStream_t stream);
void launch_prep(const PrepArgs& a, hipStream_t stream);
void launch_prep_bwd(const PrepBwdArgs& a, hipStream_t stream);

// ---- mst_eq.hip, mst_scan.hip: the EQ stage
// The zero-state pass of a SCAN1 run INSIDE the run launch (round 5; wz = nullptr: off - a zs launch went before).  Every tile forms
// its zero-state chunk end states on the matrix pipe itself, publishes its 12-state aggregate as granules and picks up the aggregates
// of the tiles before it (mst_common.h: gran_publish_vec / gran_read_vec).
struct ZsIn {
    const float* wz;    // zero-state maps, filter rows x 64 x 16 (k_prep)
    gran_t* gran;       // (signal rows, kMaxTiles1, 12) zeroed granules, indexed by the tile's position in recurrence order
    int64_t gran_near;  // the near copies follow this many granules later
    int32_t* status;    // raised to kStatusExchangeTimeout when a wait gives up (may be null)
};
// The all-pole bank's chunk states of one row family: job q = two-state system (signal row q / 12, filter q % 12)
struct ApScanJobs {
    float* z = nullptr;    // (jobs, 2, nc_pad) zero-state chunk end states
    float* s0 = nullptr;   // (jobs, 2, nc_pad) state entering every chunk (out of the carry scan)
    float* tab = nullptr;  // (filter rows x 12, kPow, 4) power tables (k_prep)
    int jobs = 0;          // 0: none
    int sh = 0;            // 64 = K 2^sh (Layout::apscan_sh)
};
// One EQ pass over one family of signal rows, filled by name: zero-state pass -> carry scan -> run.  eq_rows() below fills everything
// that lives in the workspace; the caller adds the rows that do not (the tracks, grad_tracks) and the riders it wants, and
// launch_eq_pass() picks the launches.  A null / zero member means "not there".
struct EqPass {
    int dir = EQ_FWD;                // EQ_FWD: the cascade; EQ_ADJ: its adjoint (runs backwards in time)
    // the row family
    const float* in = nullptr;       // (nsig, in_stride)
    float* out = nullptr;            // (nsig, out_stride)
    int64_t in_stride = 0, out_stride = 0;
    const float* rc = nullptr;       // row constants of the family's filter rows
    int split = 0, nsig = 0;         // see above
    int64_t n = 0;
    int nc = 0, nc_pad = 0, K = 0;   // 64-sample chunks per row, padded, chunks per carry-scan lane
    int ntiles = 0;                  // 4096-sample tiles per row
    int eq1 = 0;                     // Layout::eq1: the carries are scanned inside the zs / run kernels (SCAN1 kernels, rows of ntiles <= kMaxTiles1
                                     // tiles); the run then reads the zero-state launch's in-tile end states z directly and no carry-scan launch goes in between
    // workspace arrays of this family and direction (k_prep makes the tables)
    float* z = nullptr;              // (nsig, 12, nc_pad) zero-state chunk end states
    float* s = nullptr;              // (nsig, 12, nc_pad) state entering every chunk: out of the carry-scan launch (eq1 = 0 only)
    float* pow = nullptr;            // scan tables of the carry-scan launch
    float* pow1 = nullptr;           // in-wave scan tables (eq1)
    float* agg = nullptr;            // (nsig, 12, kMaxTiles1) tile aggregates from the zero-state launch to the run launch (eq1)
    float* wz = nullptr;             // zero-state maps, filter rows x 64 x 16 (eq1)
    // riders of the run launch
    float* zs_comp = nullptr;        // forward run of mono rows: + the gain computer and the compressor's zero-state block aggregates
    int nblk_comp = 0;               //   (nsig, nblk_comp): no separate zero-state pass over the EQ output
    float* zp = nullptr;             // forward run: + the all-pole bank of the coefficient-gradient pass, its zero-state chunk end states
                                     //   go to zp (nsig, 24, nc_pad) and the backward starts at the all-pole carry scan
    ApScanJobs scan;                 // master rows: + all-pole carry scans as extra one-wave workgroups (mst_eq.hip: k_master_run_apscan)
    // + the zero-state pass itself (round 5, ZsIn above): the tile aggregates travel as granules
    gran_t* gran = nullptr;          // (nsig, kMaxTiles1, 12) zeroed granules; null: this family and direction has none
    int64_t gran_near = 0;
    int32_t* status = nullptr;       // raised to kStatusExchangeTimeout when a wait gives up (may be null)
};
// zero-state pass, carry scan and run of p: the only place that knows the forms these take (mst_eq.hip)
void launch_eq_pass(const EqPass& p, hipStream_t stream);
// the single launches behind it.  launch_cascade: the generic kernel, zero-state pass (run = false: out, zp unused) or run
void launch_cascade(const EqPass& p, bool run, hipStream_t stream);
void launch_cascade_run_gc(const EqPass& p, bool zs_inside, hipStream_t stream);     // run + zs_comp rider
void launch_master_run_apscan(const EqPass& p, bool zs_inside, hipStream_t stream);  // run + scan rider; sh: 64 = K 2^sh
// zero-state pass of the SCAN1 path on the matrix pipe: chunk end states = W^T chunk
void launch_eq_zs_mfma(const EqPass& p, hipStream_t stream);
void launch_scan12(const EqPass& p, hipStream_t stream);  // z -> s
void launch_scan2(const float* z, float* s0, const float* tab, int split, int nc, int nc_pad, int K, int nsig, hipStream_t stream);

// The EQ stage's view of the workspace: the arrays of one row family (EQ_TRACKS: the R mono track rows; EQ_MASTER: the L/R rows of
// the bs stereo buses) in one direction.  in / out are the family's workspace signals: forward bus -> v_m and (tracks) -> u_t,
// adjoint du_m -> dbus and du_t -> (grad_tracks).
enum { EQ_TRACKS = 0, EQ_MASTER = 1 };
inline ApScanJobs allpole_rows(const Layout& L, float* ws, int family) {
    ApScanJobs j;
    const bool m = family == EQ_MASTER;
    j.z = ws + (m ? L.zP_m : L.zP_t);
    j.s0 = ws + (m ? L.sP_m : L.sP_t);
    j.tab = ws + (m ? L.powP_m : L.powP_t);
    j.jobs = (m ? 2 * L.bs : L.R) * 12;
    j.sh = L.apscan_sh;
    return j;
}
inline EqPass eq_rows(const Layout& L, float* ws, int family, int dir) {
    struct Off { int64_t rc, in, out, z, s, pow, pow1, agg, wz, gran, gran_near; };
    const int64_t none = -1, eqg_m = 2 * ((int64_t)L.R * kMaxTiles1 * kStates);  // granules are two floats wide; the master rows' follow the track rows'
    const Off o = family == EQ_TRACKS
        ? (dir == EQ_FWD ? Off{L.rc_t, none, L.u_t, L.zE_t, L.sE_t, L.powF_t, L.pow1F_t, L.aggF_t, L.wzF_t, L.eqg_f, L.eqg_nf}
                         : Off{L.rc_t, L.du_t, none, L.zA_t, L.sA_t, L.powA_t, L.pow1A_t, L.aggA_t, L.wzA_t, none, 0})
        : (dir == EQ_FWD ? Off{L.rc_m, L.bus, L.v_m, L.zE_m, L.sE_m, L.powF_m, L.pow1F_m, L.aggF_m, L.wzF_m, L.eqg_f + eqg_m, L.eqg_nf}
                         : Off{L.rc_m, L.du_m, L.dbus, L.zA_m, L.sA_m, L.powA_m, L.pow1A_m, L.aggA_m, L.wzA_m, L.eqg_b, L.eqg_nb});
    EqPass p;
    p.dir = dir;
    if (o.in != none) p.in = ws + o.in;
    if (o.out != none) p.out = ws + o.out;
    p.in_stride = p.out_stride = row_stride(L.N);
    p.rc = ws + o.rc;
    p.split = family == EQ_TRACKS ? L.R : 0;
    p.nsig = family == EQ_TRACKS ? L.R : 2 * L.bs;
    p.n = L.N;
    p.nc = L.ncE; p.nc_pad = L.ncE_pad; p.K = L.KE;
    p.ntiles = L.ntE;
    p.eq1 = L.eq1;
    p.z = ws + o.z; p.s = ws + o.s;
    p.pow = ws + o.pow; p.pow1 = ws + o.pow1;
    p.agg = ws + o.agg;
    p.wz = ws + o.wz;
    if (o.gran != none) p.gran = (gran_t*)(ws + o.gran);
    p.gran_near = o.gran_near;
    return p;
}

// ---- mst_comp.hip
struct TrackApplyArgs {
    const float* u;      // (R, stride) EQ output
    int64_t stride;
    const float* rc;     // (R, RC_STRIDE)
    const float* s0;     // (R, nc_pad) smoother start states
    float* gs;           // (R, stride) out: smoothed gain reduction in dB (saved for backward), may be null
    float* bus;          // (bs, 2, bus_stride) out
    int64_t bus_stride;
    float* mixed;        // (bs, 2, T, n) out or null
    float* fx;           // (bs, 2, bus_stride) out or null: the fx send bus sum_t send_t * mixed_t (reference stereo_bus)
    int T, nc_pad, lookahead, comp_on;
    int64_t n;
    int aligned;         // every row base / stride is 16-byte aligned: interior blocks skip all guards
};
struct MasterApplyArgs {
    const float* v;      // (bs*2, stride) master EQ output (or the raw bus when the master bus is off)
    int64_t stride;
    const float* rc;     // (bs, RC_STRIDE)
    const float* s0;     // (bs, nc_pad)
    float* gs;           // (bs, stride) or null
    float* out;          // (bs, 2, out_stride)
    int64_t out_stride;
    int nc_pad, lookahead, comp_on;
    int64_t n;
    int aligned;
    gran_t* gran;        // (bs, nblk) zeroed granules (+ their near copies gran_near granules later): the smoother's block aggregates are exchanged inside this launch; null = read s0
    int64_t gran_near;
    int32_t* status;     // raised to kStatusExchangeTimeout when an exchange wait gives up (may be null)
};
// One argument block for tracks (NCH = 1) and master (NCH = 2).
struct CompBwdArgs {
    const float* u;       // (rows*NCH, stride)  compressor input (EQ output)
    int64_t stride;
    const float* gs;      // (rows, stride) saved smoothed gain (dB)
    const float* rc;      // (rows, RC_STRIDE)
    const float* s0;      // run pass: adjoint smoother state entering each chunk from the right
    float* zq;            // (rows, nc_pad) not used by the run pass (the field keeps the kernels' argument layout)
    float* du;            // (rows*NCH, stride) out of the run pass: cotangent of the compressor input
    float* part;          // (rows, nblk, CP_COUNT) out of the run pass
    const float* gup;     // tracks: grad wrt stereo bus ; master: grad wrt mix ; (bs,2,gup_stride)
    int64_t gup_stride;
    const float* gmixed;  // tracks only: grad wrt mixed_tracks (bs,2,T,n) or null
    const float* gfx;     // tracks only: grad wrt the fx send bus (bs,2,gfx_stride) or null
    int64_t gfx_stride;
    int T, nc_pad, lookahead, comp_on;
    int64_t n;
    int aligned;
    // the run pass also forms the coefficient-gradient sums of its 2048 samples (else ep = null)
    const float* ap_s0;   // all-pole states entering every 64-sample chunk (rows, 24, ap_nc_pad)
    int ap_nc_pad;
    float* ep;            // (rows, nblkC, EP_COUNT)
    // tracks launch only: extra signal rows whose coefficient-gradient sums ride along (the two channels of every master bus: their
    // compressor adjoint ran in the master launch, all that is left is the all-pole walk over u2 = master EQ output and du2 = its cotangent)
    const float* cg2_u;   // (cg2_rows, stride)
    const float* cg2_du;  // (cg2_rows, stride)
    const float* cg2_rc;  // (cg2_rows / 2, RC_STRIDE) filter rows
    int cg2_rows;         // 0: none; signal row of extra row j = main rows + j (all-pole states, partial sums)
    gran_t* gran;         // (rows, nblk) zeroed granules (+ near copies gran_near granules later): the run pass publishes / awaits the block aggregates itself (no zs launch); null = read s0
    int64_t gran_near;
    int32_t* status;      // raised to kStatusExchangeTimeout when an exchange wait gives up (may be null)
};
void launch_apply_tracks(const TrackApplyArgs& a, int bs, hipStream_t stream);
void launch_apply_master(const MasterApplyArgs& a, int bs, hipStream_t stream);
void launch_comp_bwd(bool master, const CompBwdArgs& a, int rows, hipStream_t stream);

// ---- mst_fx.hip: the fx bus (noise-shaped reverberation on a send bus); offsets are float offsets into the workspace
struct FxPlan {
    int bs, S, taps, K, nblk, nblk_ir;
    int64_t n, Ns;
    int64_t rcfx, fx_in, wnf, ir, Xs, Hs, Ys, dXs, dHs, dir, dfx_in, fxpart, Hf, mixv, dry;
};
void launch_fx_forward(const FxPlan& p, const float* noise, const float* filters, const float* tables, float* ws, float* bus,
                       int64_t bus_stride, hipStream_t stream);
void launch_fx_backward(const FxPlan& p, const float* dbus, int64_t dbus_stride, const float* tables, float* ws, hipStream_t stream);
void launch_fx_tables(float* tables, hipStream_t stream);

}  // namespace mst
