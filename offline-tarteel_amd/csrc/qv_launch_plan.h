// qv_launch_plan.h -- which kernel a launch gets and how long its blocks' runs are: pure integer functions of the launch
// shape and a snapshot of the switches (qv_switches.h).  No HIP here: the launchers (qv_gemm.hip, qv_frontend.hip,
// qv_attention.hip) turn a plan into launches, tools/launch_plan_check.cpp runs the plans on a CPU.
#pragma once

#include "qv_limits.h"     // SUB_TT, SUB_RES_RUN, SUB_MAX_RUN, S35_TC, S35_MAX_RUN, ATT_SHORT_T
#include "qv_switches.h"

enum GemmWeights { GEMM_W_F16 = 0, GEMM_W_INT4 = 1, GEMM_W_INT8 = 2, GEMM_W_A8W8 = 3 };
// what gemm_plan reads of a GEMM call (GemmArgs in qv_kernels.h)
struct GemmShape {
    int M, N, K;
    int weights;      // GemmWeights
    bool has_bias;
    bool glu;         // the GLU epilogue (its 128-wide tile holds both halves of a channel pair: never narrow by request)
    int in_flight;    // batches the engine keeps in flight on the device
};
struct GemmPlan { bool wide, narrow; int nst, bm; };

// Tile and pipeline choice (measured per shape, tools/gemm_bench.hip):
//  * 256 x 256 tiles, one block per CU (qv_gemm256.hip), when N % 256 == 0 and the grid is large enough (see below:
//    FFN-up and QKV at B = 64 x 10 s, every N >= 512 shape at B = 256; more shapes with >= 3 batches in flight);
//  * otherwise 128-wide tiles whenever N allows, register-staged loader waves (QVERSE_GEMM_LD=0: direct global->LDS
//    loads with 2 stages at >= 400 tiles (two 64 KB blocks per CU), else 3, 4 when the K loop is long);
//  * int4 weights with too few 128-wide tiles for two blocks per CU (FFN-down, out-projection: N = 512): the consumer
//    wave of a lone block pays its dequantisation VALU in front of its own MFMAs; 64-wide tiles give every SIMD a
//    second consumer wave to interleave with.
inline GemmPlan gemm_plan(const GemmShape &g, const QvSwitches &sw) {
    const bool w4 = g.weights == GEMM_W_INT4;
    const int env_nst = sw[QV_SW_GEMM_NST], env_narrow = sw[QV_SW_GEMM_NARROW], env_ld = sw[QV_SW_GEMM_LD];
    GemmPlan p;
    p.narrow = g.N % 128 != 0;
    if (w4 && !p.narrow && (g.N / 128) * ((g.M + 127) / 128) < 400) p.narrow = true;
    if (env_narrow >= 0 && g.N % 128 == 0 && !g.glu) p.narrow = env_narrow != 0;
    const int tiles = (g.N / (p.narrow ? 64 : 128)) * ((g.M + 127) / 128);
    p.nst = tiles >= 400 ? 2 : (g.K / 64 >= 16 ? 4 : 3);
    if (p.narrow && p.nst > 3) p.nst = 3;
    if (env_nst >= 2 && env_nst <= (p.narrow ? 3 : 4)) p.nst = env_nst;
    if (env_ld == 1) p.nst = 0;
    const int t256 = sw[QV_SW_GEMM_T256];
    p.wide = false;
    p.bm = 256;
    if (t256 > 0 && g.N % 256 == 0 && g.has_bias && !(w4 && (g.K % 128 != 0 || g.K > 4096))) {
        const int tiles256 = (g.N / 256) * ((g.M + 255) / 256);
        // one batch at a time: a 256 x 256 grid must cover most of the chip (>= 160 tiles) or the 128-wide kernel's
        // 252+ blocks finish sooner; with >= 3 batches in flight the other batches' kernels take the idle CUs and
        // what counts is CU time per GEMM -- 128 tiles are enough, and the long-K shapes (FFN-down, the
        // subsampling projection: 64 tiles at B = 64 x 10 s) go wide as well (+2.3 % end to end, same-box sweep)
        const int env_min = sw[QV_SW_GEMM_MINTILES], env_min_longk = sw[QV_SW_GEMM_MINTILES_LONGK];
        const bool busy = g.in_flight >= 3;
        // (four or more batches in flight: wide tiles wherever the shape allows, +1.4 % over the 128-tile threshold)
        const int min_tiles = env_min > 0 ? env_min : g.in_flight >= 4 ? 1 : busy ? 128 : 160;
        const int min_tiles_longk = env_min_longk > 0 ? env_min_longk : busy ? 1 : 160;
        p.wide = t256 >= 2 || tiles256 >= (g.K >= 2048 ? min_tiles_longk : min_tiles);
        // Tile height (round 6).  A 192-row tile moves 17 % more operand bytes per flop, so it is only worth its rounds:
        // one batch at a time a GEMM takes ceil(tiles / 256 CUs) rounds of one tile time each (M = 24,064 = 64 clips x
        // 30 s, N = 512: 188 tiles of 256 rows = one round with 68 CUs idle, 252 tiles of 192 rows = one round of 3/4 the
        // length).  With three or more batches in flight the other batches' kernels take the idle CUs and CU time per
        // GEMM is what counts (mode 2 applies the rule there too; tools/gemm_bench + bench.py measure both).
        const int bm_mode = sw[QV_SW_GEMM_BM];
        if (p.wide && bm_mode > 0) {
            const long tiles192 = (long)(g.N / 256) * ((g.M + 191) / 192);
            const long cost256 = ((tiles256 + 255) / 256) * 256, cost192 = ((tiles192 + 255) / 256) * 192;
            if (bm_mode >= 3 || ((bm_mode == 2 || !busy) && cost192 * 108 <= cost256 * 100)) p.bm = 192;
        }
    }
    return p;
}

// The k_gemm instantiation a plan that is not wide ends in: tile width, LDS stages and loader scheme (1 = register staging,
// 0 = direct global->LDS loads) AFTER the clamps of the kernels that exist -- int8 weights and A8W8 are built 128-wide with
// register-staged loaders and two stages only, whatever the switches ask for; the GLU tile holds both halves of a channel
// pair and is never narrow; a narrow tile has at most 3 stages.  launch_gemm launches exactly this and qv_gemm_kernel_name
// prints exactly this, so the two cannot disagree (tools/launch_plan_check.cpp pins it).
struct GemmKernel { int bn, nst, ld; };
inline GemmKernel gemm_kernel(const GemmShape &g, const GemmPlan &p) {
    if (g.weights == GEMM_W_INT8 || g.weights == GEMM_W_A8W8) return {128, 2, 1};
    const int bn = p.narrow && !g.glu ? 64 : 128;
    if (p.nst == 0) return {bn, 2, 1};
    return {bn, p.nst <= 2 ? 2 : p.nst == 3 || bn == 64 ? 3 : 4, 0};
}

// Tiles per block of k_sub01, from the launch shape alone (the forward graph is keyed on the shape; no output value depends
// on it).  A CU holds two blocks, so the chip takes 512 at a time: the cost of a run length is (rounds of 512 blocks) x
// (2 x tiles + 1: a block's statistics, first mel rows and halo row cost about half a tile).  64 x 10 s = 64 x 63 tiles:
// 8 runs of 8 = 512 blocks; a small batch gets short runs and fills the chip instead.  QV_KV_SUB_RUN forces 1, 2 or
// SUB_MAX_RUN tiles, 4 forces SUB_RES_RUN (tests: the run length changes no bit).  The choice stops at SUB_RES_RUN tiles,
// the longest run whose mel rows stay resident in LDS (k_sub01<true>); a run of 4 measured like one of 8 before that
// (profiles/r09_a_run_length_sweep.txt), and resident rows take three of a run's four mel passes away.
inline int sub01_run_tiles(int batch, int t2_max, const QvSwitches &sw) {
    const int n_tiles = (t2_max + SUB_TT - 1) / SUB_TT, forced = sw[QV_KV_SUB_RUN];
    int best = 1;
    if (forced >= 1 && forced <= 4) best = forced == 3 ? SUB_MAX_RUN : forced == 4 ? SUB_RES_RUN : forced;
    else {
        long best_cost = -1;
        for (int run = 1; run <= SUB_RES_RUN; ++run) {
            const long blocks = (long)batch * ((n_tiles + run - 1) / run), cost = (blocks + 511) / 512 * (2 * run + 1);
            if (best_cost < 0 || cost < best_cost) { best = run; best_cost = cost; }
        }
    }
    return best < n_tiles ? best : (n_tiles > 0 ? n_tiles : 1);
}

// Steps of S35_TC c2 frames per block of k_sub35, from the launch shape alone (like sub01_run_tiles).  One block per CU,
// 256 CUs: the cost of a run length is (rounds of 256 blocks) x (steps + 1: a block's weight fetch and halo frame cost
// about a step).  64 x 10 s = 64 x 42 steps: 4 runs of 11 = 256 blocks.  QV_KV_SUB35 forces 1, 2 or S35_MAX_RUN steps.
inline int sub35_run_steps(int batch, int t3_max, const QvSwitches &sw) {
    const int n_steps = (t3_max + S35_TC - 1) / S35_TC, forced = sw[QV_KV_SUB35];
    int best = 1;
    if (forced >= 1 && forced <= 3) best = forced == 3 ? S35_MAX_RUN : forced;
    else {
        long best_cost = -1;
        for (int run = 1; run <= S35_MAX_RUN; ++run) {
            const long blocks = (long)batch * ((n_steps + run - 1) / run), cost = (blocks + 255) / 256 * (run + 1);
            if (best_cost < 0 || cost < best_cost) { best = run; best_cost = cost; }
        }
    }
    return best < n_steps ? best : (n_steps > 0 ? n_steps : 1);
}

// Variants of the attention kernel (tests/test_gpu_forward.py): 3 = the default (an utterance of at most ATT_SHORT_T
// frames on k_attention_short, a longer one on k_attention_ws with two heads per block), 0 = k_attention_ws with two heads per
// block for every utterance, 1 = one head per block (3 K/V stages, 256-row ring), 2 = the one-wave-per-query-tile kernel the
// specialised ones replaced, 4 = k_attention_x (round 6: four self-staging waves per (head, query group), two blocks per CU)
// for every utterance, 5 = k_attention_short + k_attention_x; 0, 1, 2 and 4 are bit-identical, so are 3 and 5.
// k_attention_x is 4-10 % faster than k_attention_ws launched back to back (tools/att_bench) and level with it inside the
// forward with batches in flight (profiles/r06_p_attention_x_same_box.log), so it stays a variant.
enum AttKernel { ATT_NONE, ATT_WS_2_2_192, ATT_WS_1_3_256, ATT_X_192, ATT_OLD };
struct AttentionPlan {
    bool run_short;   // k_attention_short first
    int rest;         // AttKernel: the kernel behind it (ATT_NONE: nothing)
    int t_short;      // utterances of at most this many frames are the short kernel's: the rest kernel leaves them alone
};
// t_min / t_max: the batch's shortest / longest utterance
inline AttentionPlan attention_plan(int variant, int t_min, int t_max) {
    if (variant == 2) return {false, ATT_OLD, 0};
    // default (3): an utterance of at most ATT_SHORT_T frames goes to k_attention_short, a longer one to the
    // wave-specialised kernel -- by its OWN length, so that its bits do not depend on the batch it travels in; a launch
    // none of whose utterances qualify is skipped
    AttentionPlan p = {false, ATT_NONE, 0};
    if (variant == 3 || variant == 5) {      // 5: k_attention_short for short utterances, k_attention_x for the longer ones
        p.t_short = ATT_SHORT_T;
        p.run_short = t_min <= ATT_SHORT_T;
        if (t_max <= ATT_SHORT_T) return p;
    }
    p.rest = variant == 4 || variant == 5 ? ATT_X_192 : variant == 1 ? ATT_WS_1_3_256 : ATT_WS_2_2_192;
    return p;
}
