// dev / test: the kernel switches (csrc/qv_switches.h) and the launch plans (csrc/qv_launch_plan.h) -- host only, no GPU.
//
//     c++ -std=c++17 -fsanitize=address,undefined tools/launch_plan_check.cpp -o launch_plan_check
//     ./launch_plan_check switches     every row of the table: environment / default, override, override -1 (prints the values
//                                      it read from THIS process's environment: the test sets it and knows what to expect)
//     ./launch_plan_check pins         plans that can be derived by hand from the comments next to the policies
//     ./launch_plan_check sweep        the plans over a grid, for comparison with a restatement of the rules
//
// Exit status 0 when every check holds; tests/test_launch_plan_host.py builds and runs it.
#include "../offline-tarteel_amd/csrc/qv_launch_plan.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

namespace {

int switches() {
    const QvSwitches env = qv_switches_env();
    CHECK(qv_switches_now() == env);                       // no override set: the environment, or the default
    for (int i = 0; i < QV_SW_COUNT; ++i) {
        const QvSwitchRow &r = QV_SWITCH_TABLE[i];
        CHECK(r.id == i && r.lo <= r.dflt && r.dflt <= r.hi && (r.parse == QV_PARSE_NONE) == (r.env == nullptr));
        printf("switch %d %s %d\n", i, r.env ? r.env : "-", env[i]);
        for (int mode : {r.hi, r.lo > 0 ? r.lo : 0, r.dflt > 0 ? r.dflt : 0}) {
            qv_switch_set(i, mode);
            QvSwitches want = env;
            want.v[i] = mode;
            CHECK(qv_switches_now() == want);              // the override wins, and moves no other row
        }
        qv_switch_set(i, -1);
        CHECK(qv_switches_now() == env);                   // -1: back to the environment
    }
    // the named setters write the rows they are named after
    for (int which = 0; which < QV_KV_COUNT; ++which) {
        qv_kernel_variant_set(which, 7);
        CHECK(qv_switches_now()[which] == 7);
        qv_kernel_variant_set(which, -5);                  // any negative mode
        CHECK(qv_switches_now() == env);
    }
    qv_kernel_variant_set(QV_KV_COUNT, 1);                 // not a kernel variant: ignored
    qv_kernel_variant_set(-1, 1);
    CHECK(qv_switches_now() == env);
    qv_attention_set_variant(4); qv_gemm_set_t256(2); qv_gemm_set_bm(3);
    QvSwitches sw = qv_switches_now(), want = env;
    want.v[QV_SW_ATT] = 4; want.v[QV_SW_GEMM_T256] = 2; want.v[QV_SW_GEMM_BM] = 3;
    CHECK(sw == want && !(sw == env));
    // a snapshot is a value: what is set after it was taken does not reach it
    qv_attention_set_variant(-1); qv_gemm_set_t256(-1); qv_gemm_set_bm(-1);
    CHECK(sw == want && qv_switches_now() == env);
    // the forward's part of a snapshot ignores exactly the switches no forward reads
    QvSwitches a = env, b = env;
    b.v[QV_KV_SPANS] ^= 1; b.v[QV_KV_CTC] ^= 1; b.v[QV_KV_FWD_GRAPH] ^= 1; b.v[QV_SW_POST_GRAPH] ^= 1;
    CHECK(!(a == b) && a.forward_part() == b.forward_part());
    for (int id : {(int)QV_KV_LOGMEL, (int)QV_KV_ORT_SUB, (int)QV_KV_SUB_RUN, (int)QV_KV_SUB35, (int)QV_SW_ATT, (int)QV_SW_GEMM_T256, (int)QV_SW_GEMM_BM,
                   (int)QV_SW_GEMM_NST, (int)QV_SW_GEMM_NARROW, (int)QV_SW_GEMM_LD}) {
        b = a;
        b.v[id] += 1;
        CHECK(!(a.forward_part() == b.forward_part()));
    }
    // the create-time rows are read again for qv_create's snapshot, every other row once per process
    const int taps = env[QV_SW_DEBUG_TAPS];
    setenv("QVERSE_DEBUG_TAPS", taps ? "0" : "1", 1); setenv("QVERSE_LOGMEL", "0", 1); setenv("QVERSE_GEMM_T256", "2", 1); setenv("QVERSE_ATT_OLD", "1", 1);
    CHECK(qv_switches_now() == env);
    want = env;
    want.v[QV_SW_DEBUG_TAPS] = !taps;
    CHECK(qv_switches_now(true) == want);
    qv_switch_set(QV_SW_DEBUG_TAPS, taps);                 // ... and an override still wins
    CHECK(qv_switches_now(true) == env);
    qv_switch_set(QV_SW_DEBUG_TAPS, -1);
    for (const QvSwitchRow &r : QV_SWITCH_TABLE)
        CHECK((r.when == QV_READ_AT_CREATE) == (r.id == QV_SW_DEBUG_TAPS || r.id == QV_SW_SUB_UNFUSED || r.id == QV_SW_SUB35_UNFUSED));
    printf("launch_plan_check: switches hold\n");
    return 0;
}

QvSwitches defaults() {
    QvSwitches sw;
    for (const QvSwitchRow &r : QV_SWITCH_TABLE) sw.v[r.id] = r.dflt;
    return sw;
}
QvSwitches with(QvSwitches sw, int id, int value) { sw.v[id] = value; return sw; }

int pins() {
    const QvSwitches d = defaults();
    // k_sub01, 64 x 10 s = 63 tiles: runs of 1 / 2 / 3 / 4 are 4032 / 2048 / 1344 / 1024 blocks = 8 / 4 / 3 / 2 rounds of 512,
    // x (2 run + 1) = 24 / 20 / 21 / 18
    CHECK(sub01_run_tiles(64, 251, d) == 4);
    CHECK(sub01_run_tiles(64, 251, with(d, QV_KV_SUB_RUN, 1)) == 1 && sub01_run_tiles(64, 251, with(d, QV_KV_SUB_RUN, 2)) == 2);
    CHECK(sub01_run_tiles(64, 251, with(d, QV_KV_SUB_RUN, 3)) == SUB_MAX_RUN && sub01_run_tiles(64, 251, with(d, QV_KV_SUB_RUN, 4)) == SUB_RES_RUN);
    CHECK(sub01_run_tiles(1, 5, with(d, QV_KV_SUB_RUN, 3)) == 2 && sub01_run_tiles(1, 0, d) == 1);   // never more than the tiles there are
    // k_sub35, 64 x 10 s = 42 steps: 4 runs of 11 make 256 blocks = 1 round x 12; runs of 10 / 14 cost 2 x 11 = 22 / 1 x 15
    CHECK(sub35_run_steps(64, 126, d) == 11);
    CHECK(sub35_run_steps(64, 126, with(d, QV_KV_SUB35, 2)) == 2 && sub35_run_steps(64, 126, with(d, QV_KV_SUB35, 3)) == S35_MAX_RUN);
    // FFN-up of 24 x 10 s: 8 x 12 = 96 tiles of 256 x 256
    const GemmShape up = {24 * 126, 2048, 512, GEMM_W_F16, true, false, 1};
    GemmPlan p = gemm_plan(up, d);
    CHECK(d[QV_SW_GEMM_T256] == 1 && !p.wide && !p.narrow && p.nst == 0);        // 96 < 160
    p = gemm_plan(up, with(with(d, QV_SW_GEMM_T256, 2), QV_SW_GEMM_BM, 0));
    CHECK(p.wide && p.bm == 256);
    p = gemm_plan(up, with(with(d, QV_SW_GEMM_T256, 2), QV_SW_GEMM_BM, 3));
    CHECK(p.wide && p.bm == 192);
    p = gemm_plan(up, with(d, QV_SW_GEMM_T256, 2));   // height mode 1: 8 x 16 tiles of 192 rows, one round of 192 against one of 256
    CHECK(p.wide && p.bm == 192);
    p = gemm_plan(up, with(d, QV_SW_GEMM_T256, 0));
    CHECK(!p.wide && !p.narrow);                                                  // f16 weights: 128-wide
    GemmShape up4 = up;
    up4.weights = GEMM_W_INT4;
    p = gemm_plan(up4, with(d, QV_SW_GEMM_T256, 0));
    CHECK(!p.wide && p.narrow);                                                   // int4: 16 x 24 = 384 < 400 tiles of 128
    // the k_gemm instantiation behind a plan (gemm_kernel): what launch_gemm launches and qv_gemm_kernel_name prints
    auto kernel = [](const GemmShape &g, const QvSwitches &sw) { return gemm_kernel(g, gemm_plan(g, sw)); };
    auto is = [](const GemmKernel &k, int bn, int nst, int ld) { return k.bn == bn && k.nst == nst && k.ld == ld; };
    const QvSwitches t0 = with(d, QV_SW_GEMM_T256, 0), lds = with(t0, QV_SW_GEMM_LD, 0);
    CHECK(is(kernel(up, t0), 128, 2, 1) && is(kernel(up4, t0), 64, 2, 1));          // the defaults: register staging
    CHECK(is(kernel(up, with(t0, QV_SW_GEMM_NARROW, 1)), 64, 2, 1) && is(kernel(up4, with(t0, QV_SW_GEMM_NARROW, 0)), 128, 2, 1));
    CHECK(is(kernel(up, with(t0, QV_SW_GEMM_NST, 3)), 128, 2, 1));                  // a stage count alone does not leave register staging
    CHECK(is(kernel(up, lds), 128, 3, 0));                                          // direct loads: 384 tiles < 400, K / 64 = 8 < 16 -> 3 stages
    CHECK(is(kernel(up, with(lds, QV_SW_GEMM_NST, 2)), 128, 2, 0) && is(kernel(up, with(lds, QV_SW_GEMM_NST, 4)), 128, 4, 0));
    CHECK(is(kernel(up, with(lds, QV_SW_GEMM_NARROW, 1)), 64, 2, 0));               // 32 x 24 = 768 tiles of 64 -> 2 stages
    CHECK(is(kernel(up, with(with(lds, QV_SW_GEMM_NARROW, 1), QV_SW_GEMM_NST, 3)), 64, 3, 0));
    CHECK(is(kernel(up, with(with(lds, QV_SW_GEMM_NARROW, 1), QV_SW_GEMM_NST, 4)), 64, 2, 0));   // 4 is not a narrow stage count: the plan's own
    GemmShape down = {420, 512, 2048, GEMM_W_F16, true, false, 1};                  // FFN-down of 420 rows: 16 tiles, K / 64 = 32 -> 4 stages
    CHECK(is(kernel(down, lds), 128, 4, 0) && is(kernel(down, with(lds, QV_SW_GEMM_NARROW, 1)), 64, 3, 0));
    down.weights = GEMM_W_INT4;
    CHECK(is(kernel(down, lds), 64, 3, 0) && is(kernel(down, with(lds, QV_SW_GEMM_NARROW, 0)), 128, 4, 0));
    CHECK(is(gemm_kernel(down, GemmPlan{false, true, 4, 256}), 64, 3, 0));          // (a narrow tile never has 4 stages, whoever made the plan)
    GemmShape glu = {420, 1024, 512, GEMM_W_F16, true, true, 1};                    // pointwise conv + GLU: never narrow
    CHECK(is(kernel(glu, with(with(lds, QV_SW_GEMM_NARROW, 1), QV_SW_GEMM_NST, 3)), 128, 3, 0));
    CHECK(is(gemm_kernel(glu, GemmPlan{false, true, 0, 256}), 128, 2, 1) && is(gemm_kernel(glu, GemmPlan{false, true, 4, 256}), 128, 4, 0));
    for (int w : {(int)GEMM_W_INT8, (int)GEMM_W_A8W8})                              // int8 weights, A8W8: one instantiation, whatever is set
        for (int n : {512, 1024})
            for (int narrow : {-1, 0, 1})
                for (int nst : {0, 2, 3, 4})
                    for (int ld : {0, 1}) {
                        const GemmShape g8 = {420, n, 512, w, true, n == 1024, 1};
                        CHECK(is(kernel(g8, with(with(with(t0, QV_SW_GEMM_NARROW, narrow), QV_SW_GEMM_NST, nst), QV_SW_GEMM_LD, ld)), 128, 2, 1));
                    }
    // attention
    AttentionPlan a = attention_plan(3, 20, ATT_SHORT_T);
    CHECK(a.run_short && a.rest == ATT_NONE);                                     // every utterance is short
    a = attention_plan(3, ATT_SHORT_T + 1, 300);
    CHECK(!a.run_short && a.rest == ATT_WS_2_2_192 && a.t_short == ATT_SHORT_T);  // none is
    a = attention_plan(3, 7, 300);
    CHECK(a.run_short && a.rest == ATT_WS_2_2_192 && a.t_short == 128);           // a mixed batch
    a = attention_plan(2, 7, 300);
    CHECK(!a.run_short && a.rest == ATT_OLD);
    a = attention_plan(4, 7, 300);
    CHECK(!a.run_short && a.rest == ATT_X_192 && a.t_short == 0);
    a = attention_plan(5, 7, 300);
    CHECK(a.run_short && a.rest == ATT_X_192 && a.t_short == ATT_SHORT_T);
    a = attention_plan(5, 7, 100);
    CHECK(a.run_short && a.rest == ATT_NONE);
    a = attention_plan(0, 7, 100);
    CHECK(!a.run_short && a.rest == ATT_WS_2_2_192 && a.t_short == 0);
    a = attention_plan(1, 7, 300);
    CHECK(!a.run_short && a.rest == ATT_WS_1_3_256 && a.t_short == 0);
    printf("launch_plan_check: pins hold\n");
    return 0;
}

void print_axis(const char *name, const std::vector<int> &v) {
    printf("%s:", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

// Grid axes in loop order (outermost first), then one character per point: gemm_plan as '0' + (wide | narrow << 1 |
// nst << 2 | (bm == 192) << 5), its kernel (gemm_kernel) as '0' + ((bn == 64) | (nst - 2) << 1 | ld << 3), a run length as
// 'a' + run - 1.
int sweep() {
    std::vector<int> Ms = {1, 2, 63, 64, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 576, 768, 1000, 1536, 1920, 3024, 3072, 4097,
                           6143, 8064, 12288, 16128, 19200, 24064, 24065, 32256, 40001, 49920, 50000};
    const std::vector<int> Ns = {192, 256, 512, 1024, 1152, 1536, 2048}, Ks = {256, 512, 2048, 2560}, weights = {GEMM_W_F16, GEMM_W_INT4, GEMM_W_INT8, GEMM_W_A8W8};
    const std::vector<int> bias_glu = {2, 0, 3};   // has_bias << 1 | glu
    const std::vector<int> in_flight = {0, 1, 2, 3, 4, 5}, t256 = {0, 1, 2}, bm = {0, 1, 2, 3};
    // QVERSE_GEMM_NST, _NARROW, _LD, _MINTILES, _MINTILES_LONGK: unset (the defaults), then set
    const int D = -1000;   // "the table's default"
    const std::vector<std::vector<int>> envs = {{D, D, D, D, D}, {D, D, D, 100, 40}, {3, 1, 0, D, D}, {4, 0, 0, 200, D}, {2, D, 0, D, 1}};
    print_axis("gemm M", Ms); print_axis("gemm N", Ns); print_axis("gemm K", Ks); print_axis("gemm weights", weights);
    print_axis("gemm bias_glu", bias_glu); print_axis("gemm in_flight", in_flight); print_axis("gemm t256", t256); print_axis("gemm bm", bm);
    const int env_ids[5] = {QV_SW_GEMM_NST, QV_SW_GEMM_NARROW, QV_SW_GEMM_LD, QV_SW_GEMM_MINTILES, QV_SW_GEMM_MINTILES_LONGK};
    std::vector<QvSwitches> env_sw;
    for (const std::vector<int> &e : envs) {
        QvSwitches sw = defaults();
        std::vector<int> shown;
        for (int i = 0; i < 5; ++i) {
            if (e[i] != D) sw.v[env_ids[i]] = e[i];
            shown.push_back(sw[env_ids[i]]);
        }
        print_axis("gemm env", shown);
        env_sw.push_back(sw);
    }
    std::string out, kernels;
    for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int w : weights) for (int bg : bias_glu) for (int inf : in_flight)
        for (int t : t256) for (int b : bm) for (QvSwitches sw : env_sw) {
            sw.v[QV_SW_GEMM_T256] = t; sw.v[QV_SW_GEMM_BM] = b;
            const GemmShape g = {M, N, K, w, (bg & 2) != 0, (bg & 1) != 0, inf};
            const GemmPlan p = gemm_plan(g, sw);
            CHECK(p.nst >= 0 && p.nst <= 4 && (p.bm == 256 || p.bm == 192));
            out.push_back((char)('0' + (p.wide | p.narrow << 1 | p.nst << 2 | (p.bm == 192) << 5)));
            const GemmKernel k = gemm_kernel(g, p);
            CHECK((k.bn == 64 || k.bn == 128) && k.nst >= 2 && k.nst <= (k.bn == 64 ? 3 : 4) && (k.ld == 0 || (k.ld == 1 && k.nst == 2)));
            kernels.push_back((char)('0' + ((k.bn == 64) | (k.nst - 2) << 1 | k.ld << 3)));
        }
    printf("gemm plans: %s\n", out.c_str());
    printf("plan kernels: %s\n", kernels.c_str());
    // the run lengths: every batch size up to 256 and every frame count an engine accepts (61 s: 1526 c1 frames, 763 c2 frames)
    const int B = 256, T2 = 1536, T3 = 768;
    for (int forced = 0; forced <= 4; ++forced) {
        const QvSwitches sw = with(defaults(), QV_KV_SUB_RUN, forced);
        out.clear();
        for (int b = 1; b <= B; ++b) for (int t = 1; t <= T2; ++t) out.push_back((char)('a' + sub01_run_tiles(b, t, sw) - 1));
        printf("sub01 batch 1..%d t2 1..%d forced %d: %s\n", B, T2, forced, out.c_str());
    }
    for (int forced = 0; forced <= 3; ++forced) {
        const QvSwitches sw = with(defaults(), QV_KV_SUB35, forced);
        out.clear();
        for (int b = 1; b <= B; ++b) for (int t = 1; t <= T3; ++t) out.push_back((char)('a' + sub35_run_steps(b, t, sw) - 1));
        printf("sub35 batch 1..%d t3 1..%d forced %d: %s\n", B, T3, forced, out.c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "switches")) return switches();
    if (!strcmp(mode, "pins")) return pins();
    if (!strcmp(mode, "sweep")) return sweep();
    fprintf(stderr, "usage: launch_plan_check switches | pins | sweep\n");
    return 2;
}
