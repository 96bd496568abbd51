// qv_switches.h -- every process-wide switch that picks a kernel or a code path: one table, one snapshot.  Pure host code
// (no HIP here): tools/launch_plan_check.cpp runs it on a CPU.
//
// A switch's value is its override if one is set (the qv_debug_* entry points; tests switch this way and not with setenv,
// which is not safe against launches from another thread), else its environment variable (read ONCE per process), else
// its default.  (Three rows are read again whenever an engine is created: QvWhen.)  Whoever launches kernels takes ONE snapshot (qv_switches_now) at entry and passes it down: a forward, its
// graph key and every launcher under it see the same values, whatever another thread sets meanwhile.
#pragma once

#include <stdlib.h>

#include <atomic>
#include <initializer_list>

// Ids 0 .. QV_KV_COUNT - 1 are qv_debug_kernel_variant's `which` codes: cross-check variants of single kernels.  Variants of
// one kernel give identical bits unless stated.
//   QV_KV_LOGMEL  (QVERSE_LOGMEL)   2 = FFT in registers, a wave walks a run of frames (k_logmel_run, default);
//                                   1 = FFT in registers, cross-lane strides over DPP / v_permlane*_swap, one wave per frame;
//                                   0 = Stockham FFT through LDS (the kernel of rounds 1-4)
//   QV_KV_ORT_SUB (QVERSE_ORT_SUB)  precision 2's conv.0: 1 = f32 matrix pipe, four channel groups per block (default); 0 = VALU
//   QV_KV_SPANS   (QVERSE_SPANS)    match_verse's span pass: 1 = prefix-shared walk per start verse (k_spans2, default); 0 = one walk per span
//   QV_KV_FWD_GRAPH (QVERSE_FWD_GRAPH) multi-context engines: 1 = a forward whose shape repeats on a context is replayed as one hipGraph
//                                   launch (default); 0 = always the plain launches
//   QV_KV_CTC     (QVERSE_CTC)      the alpha recursion of the CTC rerank: 1 = parity-specialised wave program (ctc_wave2, default);
//                                   0 = the wave program of rounds 1-5
//   QV_KV_SUB_RUN (QVERSE_SUB_RUN)  tiles of four c1 frames a block of k_sub01 walks: 0 = chosen from the launch shape (default);
//                                   1 / 2 = one / two tiles; 3 = the most a block ever walks (16, mel rows refetched per channel
//                                   group); 4 = the most with the run's mel rows resident in LDS (4)
//   QV_KV_SUB35   (no variable)     steps of three c2 frames a block of k_sub35 walks: 0 = chosen from the launch shape (default);
//                                   1 / 2 = one / two steps; 3 = the most a block ever walks (16)
// The rest:
//   QV_SW_ATT         the attention kernels (qv_debug_attention_variant; attention_plan in qv_launch_plan.h describes 0..5).  Its
//                     environment value comes from the four flags behind it, QVERSE_ATT_OLD > _HPB > _TILED > _X -> 2 / 1 / 0 / 5
//   QV_SW_GEMM_*      launch_gemm's tile and pipeline policy (gemm_plan in qv_launch_plan.h); T256 and BM have setters
//                     (qv_debug_gemm_tiles, qv_debug_gemm_tile_height), LD / NST / NARROW share one (qv_debug_gemm_pipeline)
//   QV_SW_DEBUG_TAPS, QV_SW_SUB_UNFUSED, QV_SW_SUB35_UNFUSED, QV_SW_CU_PARTITION   what qv_create looks at
//   QV_SW_POST_GRAPH  the post-logits chain as one graph launch (qv_post_run)
//   QV_SW_SKIP, QV_SW_DUP   timing experiments (qv_model.hip); the rows exist in a QV_DEV_HOOKS build only
enum {
    QV_KV_LOGMEL = 0, QV_KV_ORT_SUB = 1, QV_KV_SPANS = 2, QV_KV_FWD_GRAPH = 3, QV_KV_CTC = 4, QV_KV_SUB_RUN = 5, QV_KV_SUB35 = 6,
    QV_KV_RESERVED = 7, QV_KV_COUNT = 8,
    QV_SW_ATT = 8, QV_SW_ATT_OLD, QV_SW_ATT_HPB, QV_SW_ATT_TILED, QV_SW_ATT_X,
    QV_SW_GEMM_T256, QV_SW_GEMM_BM, QV_SW_GEMM_NST, QV_SW_GEMM_NARROW, QV_SW_GEMM_LD, QV_SW_GEMM_MINTILES, QV_SW_GEMM_MINTILES_LONGK,
    QV_SW_DEBUG_TAPS, QV_SW_SUB_UNFUSED, QV_SW_SUB35_UNFUSED, QV_SW_POST_GRAPH, QV_SW_CU_PARTITION,
#ifdef QV_DEV_HOOKS   // (a product build does not even carry the names: tests/test_capi_load.py)
    QV_SW_SKIP, QV_SW_DUP,
#endif
    QV_SW_COUNT
};

// how a row's environment variable becomes a value (the rules differ for historical reasons and stay as they are)
enum QvParse {
    QV_PARSE_NONE,    // no variable of its own
    QV_PARSE_DIGIT,   // atoi, but only if the first character is a digit -- anything else is ignored
    QV_PARSE_ATOI,    // atoi of whatever is set
    QV_PARSE_ONE      // 1 if the first character is '1', else 0
};

// when the variable is read: once per process, or -- the create-time switches a host sets between two engines, as the tests
// do -- again by every qv_create
enum QvWhen { QV_READ_ONCE, QV_READ_AT_CREATE };

// lo..hi: the values with a meaning (what the setter in qv_capi.hip accepts, where there is one); environment values are
// not clamped to it
struct QvSwitchRow { int id; const char *env; int dflt, lo, hi; QvParse parse; QvWhen when; };

inline constexpr QvSwitchRow QV_SWITCH_TABLE[QV_SW_COUNT] = {
    {QV_KV_LOGMEL, "QVERSE_LOGMEL", 2, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_ORT_SUB, "QVERSE_ORT_SUB", 1, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_SPANS, "QVERSE_SPANS", 1, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_FWD_GRAPH, "QVERSE_FWD_GRAPH", 1, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_CTC, "QVERSE_CTC", 1, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_SUB_RUN, "QVERSE_SUB_RUN", 0, 0, 15, QV_PARSE_DIGIT, QV_READ_ONCE},
    {QV_KV_SUB35, nullptr, 0, 0, 15, QV_PARSE_NONE, QV_READ_ONCE},
    {QV_KV_RESERVED, nullptr, 0, 0, 15, QV_PARSE_NONE, QV_READ_ONCE},
    {QV_SW_ATT, nullptr, 3, 0, 5, QV_PARSE_NONE, QV_READ_ONCE},
    {QV_SW_ATT_OLD, "QVERSE_ATT_OLD", 0, 0, 1, QV_PARSE_ONE, QV_READ_ONCE},
    {QV_SW_ATT_HPB, "QVERSE_ATT_HPB", 0, 0, 1, QV_PARSE_ONE, QV_READ_ONCE},
    {QV_SW_ATT_TILED, "QVERSE_ATT_TILED", 0, 0, 1, QV_PARSE_ONE, QV_READ_ONCE},
    {QV_SW_ATT_X, "QVERSE_ATT_X", 0, 0, 1, QV_PARSE_ONE, QV_READ_ONCE},
    {QV_SW_GEMM_T256, "QVERSE_GEMM_T256", 1, 0, 2, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_BM, "QVERSE_GEMM_BM", 1, 0, 3, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_NST, "QVERSE_GEMM_NST", 0, 0, 4, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_NARROW, "QVERSE_GEMM_NARROW", -1, -1, 1, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_LD, "QVERSE_GEMM_LD", 1, 0, 1, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_MINTILES, "QVERSE_GEMM_MINTILES", 0, 0, 1 << 30, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_GEMM_MINTILES_LONGK, "QVERSE_GEMM_MINTILES_LONGK", 0, 0, 1 << 30, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_DEBUG_TAPS, "QVERSE_DEBUG_TAPS", 0, 0, 1, QV_PARSE_ONE, QV_READ_AT_CREATE},
    {QV_SW_SUB_UNFUSED, "QVERSE_SUB_UNFUSED", 0, 0, 1, QV_PARSE_ONE, QV_READ_AT_CREATE},
    {QV_SW_SUB35_UNFUSED, "QVERSE_SUB35_UNFUSED", 0, 0, 1, QV_PARSE_ONE, QV_READ_AT_CREATE},
    {QV_SW_POST_GRAPH, "QVERSE_POST_GRAPH", 0, 0, 1, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_CU_PARTITION, "QVERSE_CU_PARTITION", 0, 0, 1, QV_PARSE_ATOI, QV_READ_ONCE},
#ifdef QV_DEV_HOOKS
    {QV_SW_SKIP, "QVERSE_SKIP", 0, 0, 255, QV_PARSE_ATOI, QV_READ_ONCE},
    {QV_SW_DUP, "QVERSE_DUP", 0, 0, 255, QV_PARSE_ATOI, QV_READ_ONCE},
#endif
};

// the snapshot: v[id] for every row of the table
struct QvSwitches {
    int v[QV_SW_COUNT];
    int operator[](int id) const { return v[id]; }
    bool operator==(const QvSwitches &o) const {
        for (int i = 0; i < QV_SW_COUNT; ++i)
            if (v[i] != o.v[i]) return false;
        return true;
    }
    // what a captured forward depends on: the switches nothing inside a forward reads (the post-logits variants, whether to
    // use graphs at all) are blanked, so that changing one of those does not miss the forward's graph
    QvSwitches forward_part() const {
        QvSwitches f = *this;
        for (int id : {(int)QV_KV_SPANS, (int)QV_KV_FWD_GRAPH, (int)QV_KV_CTC, (int)QV_KV_RESERVED, (int)QV_SW_POST_GRAPH}) f.v[id] = 0;
        return f;
    }
};

// THE place that reads the environment: the rows of one `when`
inline void qv_switches_read_env(QvSwitches &e, QvWhen when) {
    for (const QvSwitchRow &r : QV_SWITCH_TABLE) {
        if (r.when != when) continue;
        const char *s = r.parse == QV_PARSE_NONE ? nullptr : getenv(r.env);
        e.v[r.id] = !s ? r.dflt
                    : r.parse == QV_PARSE_DIGIT ? (s[0] >= '0' && s[0] <= '9' ? atoi(s) : r.dflt)
                    : r.parse == QV_PARSE_ATOI ? atoi(s) : s[0] == '1';
    }
    // QVERSE_ATT_OLD=1: one wave per query tile; QVERSE_ATT_HPB=1: one head per block; QVERSE_ATT_TILED=1: the
    // two-heads-per-block kernel for every utterance (no k_attention_short); QVERSE_ATT_X=1: k_attention_x instead of
    // k_attention_ws for the long utterances
    if (when == QV_READ_ONCE)
        e.v[QV_SW_ATT] = e.v[QV_SW_ATT_OLD] ? 2 : e.v[QV_SW_ATT_HPB] ? 1 : e.v[QV_SW_ATT_TILED] ? 0 : e.v[QV_SW_ATT_X] ? 5 : QV_SWITCH_TABLE[QV_SW_ATT].dflt;
}

// the environment's values as the process found them (defaults where nothing is set)
inline const QvSwitches &qv_switches_env() {
    static const QvSwitches env = [] {
        QvSwitches e;
        qv_switches_read_env(e, QV_READ_ONCE);
        qv_switches_read_env(e, QV_READ_AT_CREATE);
        return e;
    }();
    return env;
}

// the overrides, -1 = environment or default
struct QvOverrides {
    std::atomic<int> v[QV_SW_COUNT];
    QvOverrides() { for (std::atomic<int> &a : v) a.store(-1); }
};
inline QvOverrides g_qv_overrides;

inline void qv_switch_set(int id, int mode) {
    if (id >= 0 && id < QV_SW_COUNT) g_qv_overrides.v[id].store(mode < 0 ? -1 : mode);
}
// (the range checks are the C ABI's: qv_capi.hip)
inline void qv_kernel_variant_set(int which, int mode) { if (which < QV_KV_COUNT) qv_switch_set(which, mode); }
inline void qv_attention_set_variant(int mode) { qv_switch_set(QV_SW_ATT, mode); }
// tile policy of launch_gemm: 0 = 128-wide tiles only, 1 = 256 x 256 where the grid has >= 160 tiles (default), 2 = 256 x 256 wherever the shape allows; -1 = back to QVERSE_GEMM_T256 / the default
inline void qv_gemm_set_t256(int mode) { qv_switch_set(QV_SW_GEMM_T256, mode); }
// tile height of the wide kernel: 0 = 256 rows always, 1 = 192 rows where that saves a round of tiles and fewer than three batches
// are in flight (default), 2 = ... whatever is in flight, 3 = 192 rows always; -1 = back to QVERSE_GEMM_BM / the default
inline void qv_gemm_set_bm(int mode) { qv_switch_set(QV_SW_GEMM_BM, mode); }

// creating: qv_create's snapshot
inline QvSwitches qv_switches_now(bool creating = false) {
    QvSwitches sw = qv_switches_env();
    if (creating) qv_switches_read_env(sw, QV_READ_AT_CREATE);
    for (int i = 0; i < QV_SW_COUNT; ++i) {
        const int o = g_qv_overrides.v[i].load();
        if (o >= 0) sw.v[i] = o;
    }
    return sw;
}
