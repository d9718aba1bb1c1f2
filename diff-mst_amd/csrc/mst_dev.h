// mst_dev.h - developer instrumentation, compiled in by -DMST_CBR_STAMPS / -DMST_DEV_PROBE only.  A default build sees empty macros.
#pragma once

// -DMST_CBR_STAMPS (tools/cbr_timeline.py): wave 0 of every track workgroup of k_comp_bwd_run stamps the 100 MHz wall clock at its
// phase boundaries, CBR_STAMP(k); mst_debug_read_cbr_stamps copies the table out.  MST_CBR_STAMP_TABLE goes into the one translation
// unit that stamps (mst_comp.hip, inside namespace mst, in front of the kernels).
#ifdef MST_CBR_STAMPS
#define MST_CBR_STAMP_TABLE                                                                                  \
    constexpr int kStampSlots = 12, kStampWGs = 16384;                                                       \
    __device__ unsigned long long g_cbr_stamps[kStampWGs * kStampSlots];                                     \
    extern "C" int mst_debug_read_cbr_stamps(void* host, size_t bytes) {                                     \
        if (bytes > sizeof(g_cbr_stamps)) bytes = sizeof(g_cbr_stamps);                                      \
        return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cbr_stamps), bytes, 0, hipMemcpyDeviceToHost);    \
    }
#define CBR_STAMP(k)                                                                                         \
    do {                                                                                                     \
        if (!MASTER && threadIdx.x == 0) {                                                                   \
            const int wg_ = blockIdx.x + gridDim.x * blockIdx.y;                                             \
            if (wg_ < kStampWGs) g_cbr_stamps[wg_ * kStampSlots + (k)] = wall_clock64();                     \
        }                                                                                                    \
    } while (0)
#else
#define MST_CBR_STAMP_TABLE
#define CBR_STAMP(k) do {} while (0)
#endif

// -DMST_DEV_PROBE (tools/sidestream_probe.py): an event recorded in the middle of the console forward's launch sequence,
// MST_DEV_PROBE_AT(where, stream); mst_debug_set_mid_event arms it.  MST_DEV_PROBE_STATE goes into mst_console.hip at file scope.
#ifdef MST_DEV_PROBE
#define MST_DEV_PROBE_STATE                                                                                  \
    static hipEvent_t g_probe_ev = nullptr;                                                                  \
    static int g_probe_where = 0;                                                                            \
    extern "C" void mst_debug_set_mid_event(void* ev, int where) { g_probe_ev = (hipEvent_t)ev; g_probe_where = where; }
#define MST_DEV_PROBE_AT(where, stream)                                                                      \
    do {                                                                                                     \
        if (g_probe_ev && g_probe_where == (where)) (void)hipEventRecord(g_probe_ev, stream);                \
    } while (0)
#else
#define MST_DEV_PROBE_STATE
#define MST_DEV_PROBE_AT(where, stream) do {} while (0)
#endif
