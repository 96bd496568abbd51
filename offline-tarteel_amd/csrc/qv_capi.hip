// qv_capi.hip -- C ABI entry points (include/qverse.h), engine lifetime, table upload.

#include "qv_common.h"
#include "qv_kernels.h"
#include "qv_layers.h"
#include "qv_long_plan.h"
#include "qv_rows.h"
#include "qv_scan_plan.h"
#include "qv_tables_host.h"
#include "qv_trie_host.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>

static std::string g_create_error;

// ---- how many streams does the runtime actually run side by side? ---------------------------------------------------
// The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read ONCE when HIP initialises;
// streams that share a queue serialise.  An engine with four batches in flight needs a queue per context stream plus the
// caller's (14.8 k utt/s on 4 queues against 17.3 k on 8, profiles/r02_h_contexts_hwq_sweep.txt), and a host that touched
// HIP before the variable was set silently gets the default.  Instead of trusting the environment the library measures:
// four fresh streams -- what an engine with four contexts is about to create; the caller's stream and RCCL's already
// exist and hold their queues -- each run a one-wave kernel that spins for a fixed
// wall-clock time; the elapsed time over the spin time is how many of them shared a queue.  Measured
// (tools/hwq_probe.py, profiles/archive/r03_c_hwq_probe.txt): with GPU_MAX_HW_QUEUES=8 in place 7 fresh streams run side by side in
// a plain process and 4 after RCCL has created its own; on the default 4 queues only 3 do.
namespace {
__global__ void k_spin(long long ticks) {   // wall_clock64: 100 MHz
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
}  // namespace

#define QV_PROBE_STREAMS 4
// rounds = elapsed / spin time of `ns` spin kernels on `ns` fresh streams: 1 = all side by side
static double probe_rounds(int ns) {
    constexpr long long SPIN_TICKS = 40000;   // 400 us
    std::vector<hipStream_t> st(ns, nullptr);
    for (int i = 0; i < ns; ++i)
        if (hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking) != hipSuccess) return 0.0;
    for (int i = 0; i < ns; ++i) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[i], 1LL);   // warm-up: queue creation, code load
    for (int i = 0; i < ns; ++i) (void)hipStreamSynchronize(st[i]);
    double best = 1e30;
    for (int rep = 0; rep < 2; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < ns; ++i) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[i], SPIN_TICKS);
        for (int i = 0; i < ns; ++i) (void)hipStreamSynchronize(st[i]);
        best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    for (int i = 0; i < ns; ++i) (void)hipStreamDestroy(st[i]);
    return best / (SPIN_TICKS / 100.0);
}

// host calls on one engine are serialised (qv_engine::mu); a null engine falls through to the entry point's own check
#define QV_SERIALISE(e) std::unique_lock<std::recursive_mutex> qv_lock_; if (e) qv_lock_ = std::unique_lock<std::recursive_mutex>((e)->mu)

// Device-side order between consecutive calls on different caller streams (two host threads, each with its own stream,
// share the engine's workspace): wait for the previous call's tail on entry, leave a new tail on exit.
// Placement, one rule: QV_ORDERED stands behind the checks that need no device and before the call's first enqueue, in
// the entry point's own scope (the tail is recorded when that scope ends).  A call refused by those checks leaves the
// previous call's tail in place; every call that enqueues waits for it and leaves its own.
namespace {
struct QvStreamOrder {
    qv_engine *e;
    hipStream_t s;
    QvStreamOrder(qv_engine *e_, hipStream_t s_) : e(e_), s(s_) {
        if (e && e->tail_valid && e->tail_stream != s) (void)hipStreamWaitEvent(s, e->tail_ev, 0);
    }
    ~QvStreamOrder() {
        if (!e) return;
        if (!e->tail_ev && hipEventCreateWithFlags(&e->tail_ev, hipEventDisableTiming) != hipSuccess) { e->tail_ev = nullptr; return; }
        if (hipEventRecord(e->tail_ev, s) == hipSuccess) { e->tail_stream = s; e->tail_valid = true; }
    }
};
}  // namespace
#define QV_ORDERED(e, stream) QvStreamOrder qv_order_((e), (hipStream_t)(stream))

extern "C" int32_t qv_probe_concurrent_streams(void) {
    // one probe per process, also when two threads create engines at once: the mutex covers the measurement itself (two
    // probes side by side would halve each other's figure), and a failed probe (0) is not cached
    static std::mutex mu;
    static int cached = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (cached) return cached;
    const double rounds = probe_rounds(QV_PROBE_STREAMS);
    if (rounds == 0.0) return 0;
    cached = rounds < 1.5 ? QV_PROBE_STREAMS : rounds < 2.5 ? QV_PROBE_STREAMS / 2 : 1;
    return cached;
}

// dev tool (tools/hwq_probe.py): the raw figure for any number of streams, not cached
extern "C" double qv_debug_probe_rounds(int32_t n_streams) { return n_streams >= 1 && n_streams <= 32 ? probe_rounds(n_streams) : 0.0; }

static std::mutex g_create_error_mu;
void qv_set_error(qv_engine *e, const std::string &msg) {
    if (e) e->last_error = msg;   // callers hold e->mu (every entry point takes it before it can fail)
    else { std::lock_guard<std::mutex> lk(g_create_error_mu); g_create_error = msg; }
}

// The text is copied into a buffer of the CALLING thread under the engine's lock: another thread's call may replace
// (and free) the engine's string at any time, the returned pointer stays valid until this thread asks again.
extern "C" const char *qv_last_error(const qv_engine *e) {
    static thread_local std::string mine;
    if (e) {
        std::lock_guard<std::recursive_mutex> lk(const_cast<qv_engine *>(e)->mu);
        mine = e->last_error;
    } else {
        std::lock_guard<std::mutex> lk(g_create_error_mu);
        mine = g_create_error;
    }
    return mine.c_str();
}

extern "C" int qv_debug_int4_roundtrip(const float *w, int32_t N, int32_t K, float *out) {
    if (!w || !out || N < 64 || N % 64 != 0 || K < 128 || K % 128 != 0) return QV_ERR_ARG;
    std::vector<uint8_t> q((size_t)N * K / 2, 0);
    std::vector<half_t> sc((size_t)N * (K / 128) * 2);
    qv_pack_w4(w, N, K, q.data(), sc.data());
    // walk the device layout exactly as the kernel does (qv_kernels.h: GemmArgs::Wq / wscale)
    // (restated here on purpose, not qv_w4_put's address function: the round-trip tests check the packer against this walk)
    const int nk = K / 64;
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            int kt = k >> 6, c = (k & 63) >> 3, e = k & 7, p = e >> 1;
            const uint8_t *tile = q.data() + ((size_t)(n >> 6) * nk + kt) * 2048 + (size_t)(n & 63) * 32;
            uint32_t chunk;
            memcpy(&chunk, tile + 4 * (c ^ ((n >> 2) & 7)), 4);
            uint32_t pair = (chunk >> (4 * p)) & 0x000F000Fu;
            int code = (e & 1) ? (int)(pair >> 16) : (int)(pair & 0xFFFF);
            const half_t *sz = sc.data() + ((size_t)(k >> 7) * N + n) * 2;
            out[(size_t)n * K + k] = ((float)code - ((float)sz[1] - 1024.f)) * (float)sz[0];
        }
    return QV_OK;
}

extern "C" int qv_debug_int8_roundtrip(const float *w, int32_t N, int32_t K, float *out) {
    if (!w || !out || N < 64 || N % 64 != 0 || K < 64 || K % 64 != 0) return QV_ERR_ARG;
    std::vector<uint8_t> q((size_t)N * K, 0);
    std::vector<float> sc((size_t)N);
    qv_pack_w8(w, N, K, q.data(), sc.data());
    // walk the device layout exactly as the kernel does (qv_kernels.h: GemmArgs::W8 / w8scale)
    // (restated here on purpose, not the packer's address function: the round-trip tests check the packer against this walk)
    const int nk = K / 64;
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            int kt = k >> 6, c = (k & 63) >> 3;
            const uint8_t *row = q.data() + ((size_t)(n >> 6) * nk + kt) * 4096 + (size_t)(n & 63) * 64;
            int code = (int)row[((c ^ ((n >> 2) & 7)) << 3) + (k & 7)] - 128;
            out[(size_t)n * K + k] = (float)code * sc[n];
        }
    return QV_OK;
}

extern "C" const char *qv_build_info(void) {
    // the compiler is part of the contract: the GEMM loaders are inline-asm buffer loads with hand-counted s_waitcnt
    // vmcnt(N), correct for the register allocation THIS hipcc produced (tests/test_loader_hazards.py checks the code
    // objects of every build; a different compiler has to pass that test again)
    static char buf[256];
    snprintf(buf, sizeof buf, "libqverse gfx950 hip-%d.%d.%d clang-%s", HIP_VERSION_MAJOR, HIP_VERSION_MINOR, HIP_VERSION_PATCH,
             __clang_version__);
    return buf;
}

extern "C" void qv_config_default(qv_config *c) {
    memset(c, 0, sizeof *c);
    c->struct_size = (int32_t)sizeof(qv_config);
    c->device = 0;
    c->with_model = 1;
    c->precision = QV_PREC_FP16;
    c->max_batch = 64;
    c->max_samples = 480000;
    c->random_weights_seed = 20260630ull;
    c->top_text = 100;
    c->top_span_refs = 80;
    c->max_span = 6;
    c->threshold = 0.80;
    c->text_weight = 0.0;
    c->span_penalty = 0.5;
    c->skip_unused_passes = 1;
    c->n_contexts = 1;
    c->max_transcript = QV_MAX_TRANSCRIPT;
}

extern "C" int32_t qv_frames_for_samples(int64_t n) {
    int64_t t = n / 160 + 1;  // STFT center=True, hop 160
    for (int i = 0; i < 3; ++i) t = (t + 2 - 3) / 2 + 1;  // conv k3 s2 p1
    return (int32_t)t;
}

#define QV_TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// the tables file: let qv_tables_host.h read and check it and build the host arrays, upload each under its own name
static int load_tables(qv_engine *eng, const char *path) {
    HostTables h;
    std::string err;
    if (int rc = qv_read_host_tables(path, h, err)) { qv_set_error(eng, err); return rc; }
    QvTables &t = eng->tab;
    t.n_verses = h.n_verses; t.n_surah = h.n_surah; t.n_tri = h.n_tri; t.n_text = h.n_text;
    eng->h_surah = std::move(h.h_surah);
    eng->h_ayah = std::move(h.h_ayah);
#define UP(member) QV_TRY(qv_dev_upload(eng, eng->allocs, h.member.data(), h.member.size(), &t.member))
    UP(surah); UP(ayah); UP(surah_start); UP(surah_len);
    UP(clean8); UP(clean8_off);
    UP(clean); UP(clean_off); UP(clean_len); UP(nobsm_len);
    UP(alt); UP(alt_off); UP(alt_len);
    UP(nw[0]); UP(nw[1]); UP(nw[2]);
    UP(nobsm_rank);
    UP(wend_off); UP(wend); UP(len_order);
    UP(pmv); UP(pmv_off);
    UP(tri_keys); UP(tri_idf); UP(vtri_off); UP(vtri);
    UP(tri_post); UP(tri_map); UP(tri_slice);
    UP(tok_off); UP(tok); UP(tok_pfx);
    UP(piece_off); UP(piece_codes);
#undef UP
    return QV_OK;
}

// workspace, staging buffers, stream and events of execution context k
static int alloc_work(qv_engine *eng, int k, const QvSwitches &sw) {
    QvCtx &c = eng->ctx[k];
    QvWork &w = c.work;
    int B = eng->cfg.max_batch, N = eng->tab.n_verses;
    w.max_batch = B;
    w.t_cap = qv_frames_for_samples(eng->cfg.max_samples) + 2;
    size_t Bz = (size_t)B;
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz, &w.utt));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * w.t_cap, &w.frame_ids));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * w.t_cap, &w.greedy));
    const size_t maxq = (size_t)eng->max_q;   // the engine's window: pitch of q / qs, 64 bits of it per mask word
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * maxq + 64, &w.q));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * maxq + 64, &w.qs));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * 2 * QV_NSYM * (maxq / 64), &w.pm));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * N, &w.cand1));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * N * 3, &w.lcsf));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * N * 3, &w.fs));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * N, &w.lcs_p3));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * N * 3, &w.frag_list));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, (size_t)4, &w.frag_ctr));
    w.frag_cap = (int)(Bz * N * 3);
    w.search_sc = nullptr;
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.runner_idx));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.runner_score));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.top_search));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.top_search_sc));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.top_p3));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_RUNNER_CAP, &w.top_p3_sc));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_SPAN_BLOCKS, &w.span_part_score));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_SPAN_BLOCKS, &w.span_part_key));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_start));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_span));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_score));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_lead));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP * QV_MAX_SPAN, &w.cand_memb));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_loss));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * QV_CAND_CAP, &w.cand_final));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz, &w.results));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * 4, &w.packed));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz, &w.fail_list));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, (size_t)1, &w.n_fail));
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz, &c.t_dev));
    QV_HIP(hipHostMalloc((void **)&c.t_host_scratch, sizeof(int32_t) * Bz * QV_STAGE_SLOTS, hipHostMallocDefault));
    if (eng->cfg.with_model) QV_TRY(qv_dev_zeroed(eng, eng->allocs, Bz * w.t_cap * QV_VOCAB, &c.logprobs_ws));
    for (int i = 0; i < QV_STAGE_SLOTS; ++i) QV_HIP(hipEventCreateWithFlags(&c.t_copied[i], hipEventDisableTiming));
    if (eng->n_ctx > 1) {
        // QVERSE_CU_PARTITION=1 (experiment, DESIGN.md "Batches in flight"): context k's stream only sees its share of
        // the CUs of EVERY XCD (mask bit c * 8 + x = CU c of XCD x, tools/cumask_probe.hip; an XCD with an empty mask
        // would be unrestricted).  Masked streams are BLOCKING streams: the caller must not use the legacy default
        // stream for its own work or the contexts serialise behind it.  Four 64-CU partitions with 256 x 256 tiles
        // everywhere reach the same throughput as three unpartitioned batches in flight (16.6 k vs 16.6 k utt/s).
        if (sw[QV_SW_CU_PARTITION]) {
            uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const int lo = 32 * k / eng->n_ctx, hi = 32 * (k + 1) / eng->n_ctx;
            for (int cu = lo; cu < hi; ++cu)
                for (int x = 0; x < 8; ++x) mask[(cu * 8 + x) >> 5] |= 1u << ((cu * 8 + x) & 31);
            QV_HIP(hipExtStreamCreateWithCUMask(&c.stream, 8, mask));
        } else
        QV_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        QV_HIP(hipEventCreateWithFlags(&c.in_ready, hipEventDisableTiming));
        QV_HIP(hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
    }
    return QV_OK;
}

extern "C" int qv_create(const qv_config *cfg_in, qv_engine **out) {
    const qv_config *cfg = cfg_in;
    // struct_size: the layout the caller was compiled against.  Fields are only ever appended, so a shorter struct is an
    // older caller -- accepted from the first published layout (everything up to and including n_contexts) on, with the
    // fields it does not know at 0 -- and a longer one is a caller newer than this library, which is refused.
    const int32_t size_v1 = (int32_t)(offsetof(qv_config, n_contexts) + sizeof(int32_t));
    if (!cfg || !out || cfg->struct_size < size_v1 || cfg->struct_size > (int32_t)sizeof(qv_config)) {
        qv_set_error(nullptr, "qv_create: bad config (struct_size mismatch?)");
        return QV_ERR_ARG;
    }
    const QvSwitches sw = qv_switches_now(/*creating=*/true);   // debug taps, unfused cross-check paths, CU partition
    qv_engine *eng = new qv_engine();
    memset(&eng->cfg, 0, sizeof eng->cfg);
    memcpy(&eng->cfg, cfg_in, (size_t)cfg_in->struct_size);
    eng->cfg.struct_size = (int32_t)sizeof(qv_config);
    cfg = &eng->cfg;
    eng->max_q = cfg->max_transcript == 0 ? QV_MAX_TRANSCRIPT : cfg->max_transcript;
    eng->model = nullptr;
    eng->n_ctx = cfg->n_contexts < 1 ? 1 : cfg->n_contexts;
    eng->cur_ctx = eng->next_ctx = 0;
    eng->profile_stages = false;
    eng->inject_lp = nullptr;
    eng->inject_tmax = eng->inject_batch = 0;
    auto fail = [&](int rc) {
        { std::lock_guard<std::mutex> lk(g_create_error_mu); g_create_error = eng->last_error; }
        qv_destroy(eng);
        return rc;
    };
    if (eng->max_q != QV_MAX_TRANSCRIPT && eng->max_q != QV_MAX_TRANSCRIPT_WIDE) {
        eng->max_q = QV_MAX_TRANSCRIPT;
        qv_set_error(eng, "max_transcript must be 0, 1024 or 2048");
        return fail(QV_ERR_ARG);
    }
    eng->match = eng->max_q > QV_MAX_TRANSCRIPT ? &qv_match_wide : &qv_match_default;
    if (cfg->max_span < 2 || cfg->max_span > QV_MAX_SPAN) { qv_set_error(eng, "CTC_DIRECT_MAX_SPAN must be in [2,6]"); return fail(QV_ERR_ARG); }
    // c2c-direct/run.py:67 takes any float (negative weights included); only a non-finite one is refused here: inf * 0.0
    // text scores would put NaNs into the final scores and leave the winner undefined
    if (!std::isfinite(cfg->text_weight)) { qv_set_error(eng, "CTC_DIRECT_TEXT_WEIGHT must be a finite number"); return fail(QV_ERR_ARG); }
    if (cfg->top_text < 1 || cfg->top_text > QV_RUNNER_CAP - 1) { qv_set_error(eng, "CTC_DIRECT_TOP_TEXT must be in [1,127]"); return fail(QV_ERR_ARG); }
    if (cfg->top_span_refs < 0 || cfg->top_span_refs > 128) { qv_set_error(eng, "CTC_DIRECT_TOP_SPAN_REFS must be in [0,128]"); return fail(QV_ERR_ARG); }
    if (cfg->max_batch < 1 || cfg->max_samples < 400) { qv_set_error(eng, "bad capacity"); return fail(QV_ERR_ARG); }
    // the CTC rerank keeps a candidate's 2L+1 <= T states in one wave's registers: T <= 768 frames.  The
    // reference has no such limit (c2c-direct/run.py:332 only asks 2L+1 <= T); refuse the capacity instead
    // of silently dropping long candidates.
    if (qv_frames_for_samples(cfg->max_samples) + 2 > QV_MAX_T_CAP) {
        qv_set_error(eng, "max_samples above 976,000 (61 s) is not supported: the CTC rerank handles at most 768 encoder frames");
        return fail(QV_ERR_CAPACITY);
    }
    if (cfg->n_contexts > QV_MAX_CTX) { qv_set_error(eng, "n_contexts must be in [1,8]"); return fail(QV_ERR_ARG); }
    eng->knobs = {cfg->top_text, cfg->top_span_refs, cfg->max_span, cfg->threshold, cfg->text_weight,
                  cfg->span_penalty, cfg->skip_unused_passes};
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device) {
        qv_set_error(eng, "no HIP device available (libqverse needs a gfx950 GPU; there is no CPU fallback)");
        return fail(QV_ERR_HIP);
    }
    if (hipSetDevice(cfg->device) != hipSuccess) { qv_set_error(eng, "hipSetDevice failed"); return fail(QV_ERR_HIP); }
    eng->device = cfg->device;
    // The legacy default stream must own its hardware queue BEFORE the engine creates streams of its own.  A caller that
    // enqueues from the default stream (torch's current stream unless told otherwise) has qv_predict_batch_async record
    // an event there per batch; in a process whose first device work is this function, the runtime used to hand the
    // default stream -- first used later, by the table upload below -- a queue one of the context streams ends up on as
    // well, so that event sat behind ~300 queued kernels of an older batch and every new batch waited for it:
    // 4.7-4.8 ms per batch of 64 x 10 s instead of 3.5 (profiles/archive/r05_r_init_order.log; tools/sweep.py, which creates
    // its engine first, under-reported every row since round 2).  One kernel on the default stream, before the probe
    // below creates the process's first other streams, is what a process that touched the device earlier had anyway.
    // (A host thread that is inside a stream capture must not touch the legacy stream -- it would invalidate the capture or
    // be illegal in global mode -- so the warm-up is skipped then; such a host has used the device already.  The wait blocks
    // on whatever the host queued on blocking streams before: INTEGRATION.md "Creating the engine".)
    {
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        const bool capturing_ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;   // relaxed for the probe below
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        const bool legacy_capturing = hipStreamIsCapturing(nullptr, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
        if (capturing_ok) (void)hipThreadExchangeStreamCaptureMode(&mode);                    // restore the host's mode
        (void)hipGetLastError();
        if (!legacy_capturing) {
            hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, nullptr, 1LL);
            if (hipStreamSynchronize(nullptr) != hipSuccess) { qv_set_error(eng, "default-stream warm-up kernel failed"); return fail(QV_ERR_HIP); }
        }
    }
    // four and more batches in flight only pay with a hardware queue per context stream (and one for the caller); when
    // the runtime runs fewer streams side by side than that -- GPU_MAX_HW_QUEUES unset or set after HIP initialised --
    // three contexts is the best measured setting (17.0 k utt/s on 4 or 8 queues; four contexts on 4 queues: 14.8 k)
    if (eng->n_ctx >= 4 && qv_probe_concurrent_streams() < QV_PROBE_STREAMS) eng->n_ctx = 3;
    int rc = load_tables(eng, cfg->tables_path);
    if (rc) return fail(rc);
    for (int k = 0; k < eng->n_ctx; ++k) {
        rc = alloc_work(eng, k, sw);
        if (rc) return fail(rc);
    }
    {   // verse tracker workspace (qv_tracker_match)
        QvTrack &t = eng->track;
        if ((rc = qv_dev_zeroed(eng, eng->allocs, (size_t)QV_TRACK_CAP * eng->max_q + 64, &t.q)) || (rc = qv_dev_zeroed(eng, eng->allocs, (size_t)QV_TRACK_CAP * 4, &t.meta)) ||
            (rc = qv_dev_zeroed(eng, eng->allocs, (size_t)QV_TRACK_CAP * QV_TRACK_BLOCKS, &t.part_s)) ||
            (rc = qv_dev_zeroed(eng, eng->allocs, (size_t)QV_TRACK_CAP * QV_TRACK_BLOCKS, &t.part_k)) ||
            (rc = qv_dev_zeroed(eng, eng->allocs, (size_t)QV_TRACK_CAP, &t.out)))
            return fail(rc);
    }
    if (cfg->with_model) {
        rc = qv_model_create(eng, &eng->cfg, sw, &eng->model);
        if (rc) return fail(rc);
    }
    *out = eng;
    return QV_OK;
}

extern "C" void qv_destroy(qv_engine *e) {
    if (e && e->tail_ev) { (void)hipEventDestroy(e->tail_ev); e->tail_ev = nullptr; }
    if (!e) return;
    (void)hipDeviceSynchronize();
    if (e->model) qv_model_destroy(e->model);
    for (void *p : e->allocs) (void)hipFree(p);
    qv_long_free(e->long_ws);
    qv_align_long_free(e->align_long_ws);
    qv_beam_free(e);
    qv_scan_free(e);
    for (QvCtx &c : e->ctx) {
        if (c.t_host_scratch) (void)hipHostFree(c.t_host_scratch);
        for (QvMirror &m : c.mirrors) qv_mirror_free(m);
        if (c.stream) (void)hipStreamDestroy(c.stream);
        if (c.in_ready) (void)hipEventDestroy(c.in_ready);
        if (c.done) (void)hipEventDestroy(c.done);
        for (hipEvent_t e2 : c.t_copied) if (e2) (void)hipEventDestroy(e2);
        for (hipEvent_t e2 : c.stage_ev) if (e2) (void)hipEventDestroy(e2);
        for (int i = 0; i < c.n_post_graph; ++i) (void)hipGraphExecDestroy(c.post_graph[i].exec);
    }
    delete e;
}

// ---- what the entry points that run the forward share ---------------------------------------------------------------
static int need_model(qv_engine *eng) {
    if (eng->model) return QV_OK;
    qv_set_error(eng, "engine created without a model (with_model = 0)");
    return QV_ERR_NO_MODEL;
}

// The capacity rules of a batch of audio rows (every context has the same capacities): `batch` against max_batch, the
// longest row's frames -- *t_max -- against t_cap.  `prefix` opens the messages: "<entry point>: ", or "".
static int batch_in_capacity(qv_engine *eng, const char *prefix, const int64_t *lengths_host, int batch, int *t_max) {
    const QvWork &w = eng->ctx[0].work;
    if (batch > w.max_batch) { qv_set_error(eng, std::string(prefix) + "batch exceeds engine capacity"); return QV_ERR_CAPACITY; }
    int64_t lmax = 0;
    for (int b = 0; b < batch; ++b) lmax = std::max(lmax, lengths_host[b]);
    *t_max = qv_frames_for_samples(lmax);
    if (*t_max > w.t_cap) { qv_set_error(eng, std::string(prefix) + "audio longer than engine capacity"); return QV_ERR_CAPACITY; }
    return QV_OK;
}

// Entry points that run on the caller's stream through the workspace of ctx[cur_ctx] (a single text, a forward): with
// batches in flight, wait until no internal stream is still using a workspace.
static int quiesce_contexts(qv_engine *eng) {
    if (eng->n_ctx > 1)
        for (int k = 0; k < eng->n_ctx; ++k)
            if (eng->ctx[k].busy) QV_HIP(hipEventSynchronize(eng->ctx[k].done));
    return QV_OK;
}

// A forward on the caller's stream writes the current context's log-prob workspace: no batch may be in flight on it, and
// the batch those log-probs belonged to can no longer be aligned.  Returns that context.
static int claim_logprobs_ws(qv_engine *eng, QvCtx **c) {
    QV_TRY(quiesce_contexts(eng));
    *c = &eng->ctx[eng->cur_ctx];
    if ((*c)->al_lp == (*c)->logprobs_ws) (*c)->al_lp = nullptr;
    return QV_OK;
}

// ... and the forward itself: the rows' log-probs in (*c)->logprobs_ws, their frame counts in t_out
static int forward_into_ws(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int batch, int64_t n_max, int t_max,
                           hipStream_t stream, QvCtx **c, std::vector<int32_t> &t_out) {
    QV_TRY(claim_logprobs_ws(eng, c));
    t_out.resize(batch);
    return qv_model_forward(eng, eng->model, eng->cur_ctx, audio_dev, lengths_host, batch, n_max, (*c)->logprobs_ws, t_max, t_out.data(),
                            stream, /*zero_pad_rows=*/false);
}

extern "C" int qv_forward(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch,
                          int64_t n_max, float *logprobs_dev, int32_t t_max, int32_t *t_out_host, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    QV_ORDERED(eng, stream);
    return qv_model_forward(eng, eng->model, eng->cur_ctx, audio_dev, lengths_host, batch, n_max, logprobs_dev, t_max,
                            t_out_host, (hipStream_t)stream, /*zero_pad_rows=*/true);
}

// what qv_align_results_ctx aligns against: the log-probs the context's batch was just decoded from
static void align_note(QvCtx &c, const float *lp, int t_max, int batch, hipStream_t stream) {
    c.al_lp = lp; c.al_tmax = t_max; c.al_batch = batch; c.al_stream = stream;
}

extern "C" int qv_decode_retrieve_rerank_async(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch,
                                               int32_t t_max, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || !lp || !t_host || batch < 1) return QV_ERR_ARG;
    QV_ORDERED(eng, stream);
    QvCtx &c = eng->ctx[eng->cur_ctx];
    qv_stage_mark(eng, c, 0, (hipStream_t)stream);   // no forward in this call: forward = 0
    qv_stage_mark(eng, c, 1, (hipStream_t)stream);
    int rc = qv_post_run(eng, c, lp, t_max, t_host, batch, (hipStream_t)stream);
    if (rc == QV_OK) align_note(c, lp, t_max, batch, (hipStream_t)stream);
    return rc;
}

void qv_stage_mark(qv_engine *eng, QvCtx &c, int i, hipStream_t s) {
    if (!eng->profile_stages) return;
    if (!c.stage_ev[i]) return;
    if (i == 0) c.stage_valid = false;
    if (hipEventRecord(c.stage_ev[i], s) == hipSuccess && i == 4) c.stage_valid = true;
}

extern "C" int qv_profile_inject_logprobs(qv_engine *eng, const float *logprobs_dev, int32_t t_max, const int32_t *t_host, int32_t batch) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!logprobs_dev) { eng->inject_lp = nullptr; eng->inject_batch = 0; return QV_OK; }
    if (!t_host || batch < 1 || t_max < 1 || t_max > eng->ctx[eng->cur_ctx].work.t_cap) { qv_set_error(eng, "qv_profile_inject_logprobs: bad shape"); return QV_ERR_ARG; }
    eng->inject_t.assign(t_host, t_host + batch);
    eng->inject_lp = logprobs_dev;
    eng->inject_tmax = t_max;
    eng->inject_batch = batch;
    return QV_OK;
}

extern "C" int qv_profile_stages(qv_engine *eng, int32_t enable) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (enable)
        for (int k = 0; k < eng->n_ctx; ++k)
            for (hipEvent_t &e : eng->ctx[k].stage_ev)
                if (!e) QV_HIP(hipEventCreate(&e));
    eng->profile_stages = enable != 0;
    return QV_OK;
}

extern "C" int qv_stage_times(qv_engine *eng, int32_t k, float *ms4) {
    QV_SERIALISE(eng);
    if (!eng || !ms4 || k < 0 || k >= eng->n_ctx) return QV_ERR_ARG;
    QvCtx &c = eng->ctx[k];
    if (!c.stage_valid) { qv_set_error(eng, "qv_stage_times: no profiled batch on this context (qv_profile_stages first)"); return QV_ERR_ARG; }
    QV_HIP(hipEventSynchronize(c.stage_ev[4]));
    for (int i = 0; i < 4; ++i) QV_HIP(hipEventElapsedTime(&ms4[i], c.stage_ev[i], c.stage_ev[i + 1]));
    return QV_OK;
}

// results (and greedy ids) of context c's last batch, copied on `stream`; SYNCHRONOUS
static int fetch_results(qv_engine *eng, QvCtx &c, int batch, int t_max, qv_result *res, int32_t *greedy_host, hipStream_t stream) {
    if (!res || batch < 1 || batch > c.work.max_batch) return QV_ERR_ARG;
    QV_HIP(hipMemcpyAsync(res, c.work.results, sizeof(qv_result) * batch, hipMemcpyDeviceToHost, stream));
    if (greedy_host) {
        int tc = c.work.t_cap;
        int w = t_max < tc ? t_max : tc;
        QV_HIP(hipMemcpy2DAsync(greedy_host, sizeof(int32_t) * t_max, c.work.greedy, sizeof(int32_t) * tc,
                                sizeof(int32_t) * w, batch, hipMemcpyDeviceToHost, stream));
    }
    QV_HIP(hipStreamSynchronize(stream));
    for (int b = 0; b < batch; ++b) {
        // authoritative score of a CTC winner: math.exp(-ctc_norm_loss) in host double libm,
        // exactly what mixed/run.py:103-107 evaluates
        if (res[b].source == QV_SOURCE_CTC) res[b].score = exp(-(double)res[b].ctc_norm_loss);
        if (res[b].flags & QV_FLAG_TRANSCRIPT_TRUNCATED) { res[b].surah = res[b].ayah = res[b].ayah_end = 0; }
    }
    return QV_OK;
}

extern "C" int qv_fetch_results(qv_engine *eng, int32_t batch, int32_t t_max, qv_result *res, int32_t *greedy_host,
                                void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_ORDERED(eng, stream);
    return fetch_results(eng, eng->ctx[eng->cur_ctx], batch, t_max, res, greedy_host, (hipStream_t)stream);
}

extern "C" int qv_decode_retrieve_rerank(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch,
                                         int32_t t_max, qv_result *res, int32_t *greedy_host, void *stream) {
    QV_SERIALISE(eng);
    int rc = qv_decode_retrieve_rerank_async(eng, lp, t_host, batch, t_max, stream);
    if (rc) return rc;
    return qv_fetch_results(eng, batch, t_max, res, greedy_host, stream);
}

extern "C" int qv_predict_batch_async(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host,
                                      int32_t batch, int64_t n_max, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    int t_max;
    QV_TRY(batch_in_capacity(eng, "", lengths_host, batch, &t_max));
    QV_ORDERED(eng, stream);
    std::vector<int32_t> t_out(batch);
    hipStream_t run = (hipStream_t)stream;
    if (eng->n_ctx > 1) {
        // rotate to the next context; the host blocks only if that context's previous batch is
        // still in flight (bounds the queue and protects its pinned staging buffers)
        const int k = eng->next_ctx;
        eng->next_ctx = (k + 1) % eng->n_ctx;
        QvCtx &c = eng->ctx[k];
        if (c.busy) QV_HIP(hipEventSynchronize(c.done));
        eng->cur_ctx = k;
        QV_HIP(hipEventRecord(c.in_ready, (hipStream_t)stream));
        QV_HIP(hipStreamWaitEvent(c.stream, c.in_ready, 0));
        run = c.stream;
    }
    QvCtx &c = eng->ctx[eng->cur_ctx];
    qv_stage_mark(eng, c, 0, run);
    int rc = qv_model_forward(eng, eng->model, eng->cur_ctx, audio_dev, lengths_host, batch, n_max, c.logprobs_ws, t_max,
                              t_out.data(), run, /*zero_pad_rows=*/false, /*may_graph=*/eng->n_ctx > 1);
    if (rc) return rc;
    qv_stage_mark(eng, c, 1, run);
    if (eng->inject_lp) {
        if (batch > eng->inject_batch) { qv_set_error(eng, "injected log-probs hold fewer utterances than the batch"); return QV_ERR_ARG; }
        rc = qv_post_run(eng, c, eng->inject_lp, eng->inject_tmax, eng->inject_t.data(), batch, run);
        if (rc == QV_OK) align_note(c, eng->inject_lp, eng->inject_tmax, batch, run);
    } else {
        rc = qv_post_run(eng, c, c.logprobs_ws, t_max, t_out.data(), batch, run);
        if (rc == QV_OK) align_note(c, c.logprobs_ws, t_max, batch, run);
    }
    if (rc) return rc;
    if (eng->n_ctx > 1) {
        QV_HIP(hipEventRecord(c.done, c.stream));
        c.busy = true;
    }
    return QV_OK;
}

extern "C" int qv_predict_batch_async_ctx(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch,
                                          int64_t n_max, void *stream, int32_t *ctx_out) {
    QV_SERIALISE(eng);   // (recursive: the call below takes it again) -- the context id is read under the same lock hold
    int rc = qv_predict_batch_async(eng, audio_dev, lengths_host, batch, n_max, stream);
    if (rc == QV_OK && ctx_out) *ctx_out = eng->cur_ctx;
    return rc;
}

extern "C" int qv_predict_batch(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch,
                                int64_t n_max, qv_result *res, int32_t *greedy_host, void *stream) {
    QV_SERIALISE(eng);
    int rc = qv_predict_batch_async(eng, audio_dev, lengths_host, batch, n_max, stream);
    if (rc) return rc;
    const int last_tmax = eng->ctx[eng->cur_ctx].last_tmax;
    if (eng->n_ctx > 1) return qv_fetch_results_ctx(eng, eng->cur_ctx, batch, last_tmax, res, greedy_host);
    return qv_fetch_results(eng, batch, last_tmax, res, greedy_host, stream);
}

static int fir_for(qv_engine *eng, const float *taps, int32_t n_taps, int32_t up, const qv_engine::Fir **out);

extern "C" int qv_upfirdn(qv_engine *eng, const float *x_dev, int64_t n_in, const float *taps, int32_t n_taps, int32_t up,
                          int32_t down, int64_t m0, int64_t n_out, float *y_dev, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || !x_dev || !taps || !y_dev || n_in < 1 || n_taps < 1 || up < 1 || down < 1 || m0 < 0 || n_out < 0) return QV_ERR_ARG;
    QV_ORDERED(eng, stream);
    const qv_engine::Fir *fir = nullptr;
    QV_TRY(fir_for(eng, taps, n_taps, up, &fir));
    launch_upfirdn(x_dev, n_in, fir->hflip_dev, fir->P, up, down, m0, n_out, y_dev, (hipStream_t)stream);
    QV_HIP(hipGetLastError());
    return QV_OK;
}

// the per-phase, time-reversed filter rows of (taps, up), uploaded once per distinct filter
static int fir_for(qv_engine *eng, const float *taps, int32_t n_taps, int32_t up, const qv_engine::Fir **out) {
    for (const auto &f : eng->firs)
        if (f.up == up && (int)f.taps.size() == n_taps && memcmp(f.taps.data(), taps, sizeof(float) * n_taps) == 0) { *out = &f; return QV_OK; }
    int P = (n_taps + up - 1) / up;
    std::vector<float> hf((size_t)up * P, 0.f);
    for (int t = 0; t < up; ++t)
        for (int j = 0; j < P; ++j) {
            int k = t + up * (P - 1 - j);
            if (k < n_taps) hf[(size_t)t * P + j] = taps[k];
        }
    float *d = nullptr;
    QV_TRY(qv_dev_zeroed(eng, eng->allocs, hf.size(), &d));
    QV_HIP(hipMemcpy(d, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice));
    eng->firs.push_back({up, std::vector<float>(taps, taps + n_taps), d, P});
    *out = &eng->firs.back();
    return QV_OK;
}

// row table of a resampling call: [QV_RESAMPLE_ROWS] int64 lengths + int32 source rows, one slot of a small ring per call,
// allocated on first use (the copies into it are issued from pageable memory: the runtime stages them before the entry
// point returns, so the host vectors may go away)
static int resample_slot(qv_engine *eng, unsigned char **slot) {
    if (!eng->resample_tab) QV_TRY(qv_dev_zeroed(eng, eng->allocs, (size_t)QV_RESAMPLE_SLOTS * QV_RESAMPLE_ROWS * 12, &eng->resample_tab));
    *slot = eng->resample_tab + (size_t)(eng->resample_at++ % QV_RESAMPLE_SLOTS) * QV_RESAMPLE_ROWS * 12;
    return QV_OK;
}

extern "C" int qv_upfirdn_batch(qv_engine *eng, const float *x_dev, int64_t x_pitch, const int32_t *src_rows_host,
                                const int64_t *n_in_host, int32_t rows, const float *taps, int32_t n_taps, int32_t up, int32_t down,
                                int64_t m0, float *y_dev, int64_t y_pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || !x_dev || !n_in_host || !taps || !y_dev || rows < 1 || rows > QV_RESAMPLE_ROWS || n_taps < 1 || up < 1 || down < 1 || m0 < 0 ||
        x_pitch < 1 || y_pitch < 1)
        return QV_ERR_ARG;
    for (int r = 0; r < rows; ++r) {
        if (n_in_host[r] < 1 || n_in_host[r] > x_pitch) { qv_set_error(eng, "qv_upfirdn_batch: a row's length is outside [1, x_pitch]"); return QV_ERR_ARG; }
        if ((n_in_host[r] * up + down - 1) / down > y_pitch) { qv_set_error(eng, "qv_upfirdn_batch: y_pitch is shorter than a row's output"); return QV_ERR_ARG; }
        if (src_rows_host && src_rows_host[r] < 0) return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    const qv_engine::Fir *fir = nullptr;
    QV_TRY(fir_for(eng, taps, n_taps, up, &fir));
    unsigned char *slot = nullptr;
    QV_TRY(resample_slot(eng, &slot));
    hipStream_t s = (hipStream_t)stream;
    QV_HIP(hipMemcpyAsync(slot, n_in_host, sizeof(int64_t) * rows, hipMemcpyHostToDevice, s));
    int32_t *src_dev = nullptr;
    if (src_rows_host) {
        src_dev = (int32_t *)(slot + (size_t)QV_RESAMPLE_ROWS * 8);
        QV_HIP(hipMemcpyAsync(src_dev, src_rows_host, sizeof(int32_t) * rows, hipMemcpyHostToDevice, s));
    }
    launch_upfirdn_rows(x_dev, x_pitch, src_dev, (const int64_t *)slot, rows, fir->hflip_dev, fir->P, up, down, m0, y_dev, y_pitch, s);
    QV_HIP(hipGetLastError());
    return QV_OK;
}

extern "C" int qv_mixdown_batch(qv_engine *eng, const float *x_dev, int64_t x_pitch, const int64_t *n_frames_host, int32_t rows,
                                int32_t channels, float *y_dev, int64_t y_pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || !x_dev || !n_frames_host || !y_dev || rows < 1 || rows > QV_RESAMPLE_ROWS || channels < 1 || channels > 64) return QV_ERR_ARG;
    int64_t mx = 0;
    for (int r = 0; r < rows; ++r) {
        if (n_frames_host[r] < 0 || n_frames_host[r] * channels > x_pitch || n_frames_host[r] > y_pitch) return QV_ERR_ARG;
        mx = n_frames_host[r] > mx ? n_frames_host[r] : mx;
    }
    QV_ORDERED(eng, stream);
    unsigned char *slot = nullptr;
    QV_TRY(resample_slot(eng, &slot));
    hipStream_t s = (hipStream_t)stream;
    QV_HIP(hipMemcpyAsync(slot, n_frames_host, sizeof(int64_t) * rows, hipMemcpyHostToDevice, s));
    launch_mixdown(x_dev, x_pitch, (const int64_t *)slot, rows, channels, y_dev, y_pitch, mx, s);
    QV_HIP(hipGetLastError());
    return QV_OK;
}

extern "C" const int32_t *qv_packed_results_dev(qv_engine *eng) { return eng ? eng->ctx[eng->cur_ctx].work.packed : nullptr; }

extern "C" int32_t qv_max_transcript(const qv_engine *eng) { return eng ? eng->max_q : 0; }   // fixed at qv_create
extern "C" int32_t qv_context_count(const qv_engine *eng) { return eng ? eng->n_ctx : 0; }   // fixed at qv_create
extern "C" int32_t qv_last_context(const qv_engine *eng) {
    if (!eng) return -1;
    std::lock_guard<std::recursive_mutex> lk(const_cast<qv_engine *>(eng)->mu);
    return eng->cur_ctx;
}

extern "C" int qv_wait_ctx(qv_engine *eng, int32_t k) {
    QV_SERIALISE(eng);
    if (!eng || k < 0 || k >= eng->n_ctx) return QV_ERR_ARG;
    QvCtx &c = eng->ctx[k];
    if (eng->n_ctx > 1) {
        if (c.busy) QV_HIP(hipEventSynchronize(c.done));
    } else {
        QV_HIP(hipDeviceSynchronize());   // single-context engines run on the caller's stream, which we were not given
    }
    return QV_OK;
}

extern "C" const int32_t *qv_packed_results_ctx(qv_engine *eng, int32_t k, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || k < 0 || k >= eng->n_ctx) return nullptr;
    QvCtx &c = eng->ctx[k];
    if (eng->n_ctx > 1 && c.busy && hipStreamWaitEvent((hipStream_t)stream, c.done, 0) != hipSuccess) return nullptr;
    return c.work.packed;
}

extern "C" int qv_fetch_results_ctx(qv_engine *eng, int32_t k, int32_t batch, int32_t t_max, qv_result *res,
                                    int32_t *greedy_host) {
    QV_SERIALISE(eng);
    if (!eng || k < 0 || k >= eng->n_ctx) return QV_ERR_ARG;
    if (eng->n_ctx == 1) QV_HIP(hipDeviceSynchronize());  // the batch ran on a caller stream we were not given
    // on the context's own stream, so the copy is ordered after its batch
    // (Not qv_rows.h::qv_stream_behind_batch, here and in qv_debug_transcript_codes: that rule also joins the device when
    // the batch was decoded on a stream other than the context's own -- qv_decode_retrieve_rerank_async on an engine with
    // batches in flight -- which these two calls never did.)
    hipStream_t stream = eng->n_ctx > 1 ? eng->ctx[k].stream : nullptr;
    QV_ORDERED(eng, stream);
    return fetch_results(eng, eng->ctx[k], batch, t_max, res, greedy_host, stream);
}

// How a call on context k's last batch opens: k names a context and `batch` rows fit its workspace.  `rest_ok` and `rule`
// are the caller's other argument rules and the words for them; one QV_ERR_ARG message covers them and the context.
static int ctx_batch_args(qv_engine *eng, const char *who, int k, int batch, bool rest_ok, const char *rule) {
    if (k < 0 || k >= eng->n_ctx || batch < 1 || !rest_ok) { qv_set_error(eng, std::string(who) + ": " + rule); return QV_ERR_ARG; }
    if (batch > eng->ctx[k].work.max_batch) { qv_set_error(eng, std::string(who) + ": batch exceeds engine capacity"); return QV_ERR_CAPACITY; }
    return QV_OK;
}

// the transcript k_decode left in the workspace (rows of eng->max_q codes: the pitch of the kernel set the engine runs)
extern "C" int qv_debug_transcript_codes(qv_engine *eng, int32_t k, int32_t batch, uint8_t *codes_host, int32_t pitch,
                                         int32_t *len_host, int32_t *words_host) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(ctx_batch_args(eng, "qv_debug_transcript_codes", k, batch, codes_host && len_host && words_host && pitch >= eng->max_q,
                          "bad context, null argument, empty batch or pitch < qv_max_transcript"));
    QvCtx &c = eng->ctx[k];
    if (!c.al_lp || batch > c.al_batch) {
        qv_set_error(eng, "qv_debug_transcript_codes: the context holds no batch of that size (ask before the context is reused)");
        return QV_ERR_ARG;
    }
    if (eng->n_ctx == 1) QV_HIP(hipDeviceSynchronize());  // the batch ran on a caller stream we were not given
    hipStream_t stream = eng->n_ctx > 1 ? c.stream : nullptr;
    QV_ORDERED(eng, stream);
    std::vector<QvUtt> utt(batch);
    std::vector<uint8_t> q((size_t)batch * eng->max_q);
    QV_HIP(hipMemcpyAsync(utt.data(), c.work.utt, sizeof(QvUtt) * batch, hipMemcpyDeviceToHost, stream));
    QV_HIP(hipMemcpyAsync(q.data(), c.work.q, q.size(), hipMemcpyDeviceToHost, stream));
    QV_HIP(hipStreamSynchronize(stream));
    for (int b = 0; b < batch; ++b) {
        const int n = utt[b].q_len;
        if (n < 0 || n > eng->max_q) { qv_set_error(eng, "qv_debug_transcript_codes: q_len outside the window"); return QV_ERR_HIP; }
        memcpy(codes_host + (size_t)b * pitch, q.data() + (size_t)b * eng->max_q, (size_t)n);
        len_host[b] = n;
        words_host[b] = utt[b].q_words;
    }
    return QV_OK;
}

extern "C" int qv_debug_retrieve(qv_engine *eng, const uint8_t *codes_host, int32_t n_codes, int32_t *base_start,
                                 int32_t *base_span, double *base_score, int32_t *cand_start, int32_t *cand_span,
                                 double *cand_score, int32_t cand_cap, int32_t *n_cand, int32_t *runner_idx,
                                 double *runner_score, int32_t *n_runners, void *stream_) {
    QV_SERIALISE(eng);
    hipStream_t stream = (hipStream_t)stream_;
    if (!eng) return QV_ERR_ARG;
    QV_ORDERED(eng, stream);
    QvCtx &c = eng->ctx[eng->cur_ctx];
    c.al_lp = nullptr;   // utt[0] of this workspace is about to be overwritten
    int rc = qv_post_debug_retrieve(eng, c, codes_host, n_codes, stream);
    if (rc) return rc;
    QvUtt u;
    QV_HIP(hipMemcpy(&u, c.work.utt, sizeof(QvUtt), hipMemcpyDeviceToHost));
    *base_start = u.base_start; *base_span = u.base_span; *base_score = u.base_score;
    int n = u.n_cand < cand_cap ? u.n_cand : cand_cap;
    *n_cand = u.n_cand;
    if (n > 0) {
        QV_HIP(hipMemcpy(cand_start, c.work.cand_start, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        QV_HIP(hipMemcpy(cand_span, c.work.cand_span, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        QV_HIP(hipMemcpy(cand_score, c.work.cand_score, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    *n_runners = u.n_runners;
    if (u.n_runners > 0) {
        QV_HIP(hipMemcpy(runner_idx, c.work.runner_idx, sizeof(int32_t) * u.n_runners, hipMemcpyDeviceToHost));
        QV_HIP(hipMemcpy(runner_score, c.work.runner_score, sizeof(double) * u.n_runners, hipMemcpyDeviceToHost));
    }
    return QV_OK;
}

extern "C" int qv_tracker_match(qv_engine *eng, const uint8_t *codes_host, const int32_t *offsets_host,
                                const int32_t *n_words_host, const int32_t *bonus_verse_host, int32_t batch,
                                qv_track_match *out_host, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (batch < 0 || !offsets_host || !n_words_host || !bonus_verse_host || !out_host || (batch > 0 && !codes_host)) {
        qv_set_error(eng, "qv_tracker_match: null argument");
        return QV_ERR_ARG;
    }
    for (int b = 0; b < batch; ++b) {
        int n = offsets_host[b + 1] - offsets_host[b];
        if (n < 0 || bonus_verse_host[b] >= eng->tab.n_verses || n_words_host[b] < 0) {
            qv_set_error(eng, "qv_tracker_match: bad offsets / word count / bonus verse");
            return QV_ERR_ARG;
        }
        if (n > eng->max_q) { qv_set_error(eng, "qv_tracker_match: text longer than the engine's max_transcript"); return QV_ERR_CAPACITY; }
    }
    QV_ORDERED(eng, stream);
    return qv_post_tracker_match(eng, codes_host, offsets_host, n_words_host, bonus_verse_host, batch, out_host,
                                 (hipStream_t)stream);
}

extern "C" int qv_match_verse(qv_engine *eng, const uint8_t *codes_host, int32_t n_codes, int32_t n_bonus,
                              const int32_t *bonus_verse, const double *bonus_value, int32_t max_span, int32_t *start,
                              int32_t *span, double *score, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (n_codes < 0 || (n_codes > 0 && !codes_host) || n_bonus < 0 || n_bonus > 3 || (n_bonus > 0 && (!bonus_verse || !bonus_value)) ||
        max_span < 2 || max_span > 8 || !start || !span || !score) {
        qv_set_error(eng, "qv_match_verse: bad argument (n_bonus in [0,3], max_span in [2,8])");
        return QV_ERR_ARG;
    }
    for (int i = 0; i < n_bonus; ++i)
        if (bonus_verse[i] < 0 || bonus_verse[i] >= eng->tab.n_verses) { qv_set_error(eng, "qv_match_verse: bonus verse out of range"); return QV_ERR_ARG; }
    if (n_codes > eng->max_q) { qv_set_error(eng, "qv_match_verse: text longer than the engine's max_transcript"); return QV_ERR_CAPACITY; }
    QV_ORDERED(eng, stream);
    QV_TRY(quiesce_contexts(eng));
    QvCtx &c = eng->ctx[eng->cur_ctx];
    c.al_lp = nullptr;   // utt[0] of this workspace is about to be overwritten
    int rc = qv_post_match_verse(eng, c, codes_host, n_codes, n_bonus, bonus_verse, bonus_value, max_span, (hipStream_t)stream);
    if (rc) return rc;
    QvUtt u;
    QV_HIP(hipMemcpy(&u, c.work.utt, sizeof(QvUtt), hipMemcpyDeviceToHost));
    *start = u.base_start; *span = u.base_span; *score = u.base_score;
    return QV_OK;
}

extern "C" int qv_debug_ctc_loss(qv_engine *eng, const float *lp, int32_t T, const uint16_t *tg, const int32_t *lens,
                                 int32_t n, float *loss_host, void *stream) {
    QV_SERIALISE(eng);
    if (!eng || n < 1) return QV_ERR_ARG;
    QV_ORDERED(eng, stream);
    return qv_post_debug_ctc(eng, lp, T, tg, lens, n, loss_host, (hipStream_t)stream);
}

// ---- forced alignment (qv_align.hip) --------------------------------------------------------------------------------
extern "C" int qv_align(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch, int32_t t_max,
                        const uint16_t *targets_host, const int32_t *lens_host, qv_align_info *info_host, int16_t *first_host,
                        int16_t *last_host, float *logp_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!lp || !t_host || !lens_host || !info_host || !first_host || !last_host || !logp_host || batch < 1 || t_max < 1 ||
        pitch < QV_ALIGN_MAX_TOKENS) {
        qv_set_error(eng, "qv_align: null argument, empty batch or pitch < QV_ALIGN_MAX_TOKENS");
        return QV_ERR_ARG;
    }
    int64_t total = 0;
    for (int b = 0; b < batch; ++b) total += lens_host[b] > 0 ? lens_host[b] : 0;
    if (total > 0 && !targets_host) { qv_set_error(eng, "qv_align: targets_host is null"); return QV_ERR_ARG; }
    QV_ORDERED(eng, stream);
    return qv_align_explicit(eng, eng->ctx[eng->cur_ctx], lp, t_host, batch, t_max, targets_host, lens_host, info_host, first_host,
                             last_host, logp_host, pitch, (hipStream_t)stream);
}

extern "C" int qv_align_results_ctx(qv_engine *eng, int32_t k, int32_t batch, qv_align_info *info_host, uint16_t *ids_host,
                                    int16_t *first_host, int16_t *last_host, float *logp_host, int32_t pitch) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(ctx_batch_args(eng, "qv_align_results_ctx", k, batch,
                          info_host && ids_host && first_host && last_host && logp_host && pitch >= QV_ALIGN_MAX_TOKENS,
                          "bad context, null argument, empty batch or pitch < QV_ALIGN_MAX_TOKENS"));
    return qv_align_results(eng, k, batch, info_host, ids_host, first_host, last_host, logp_host, pitch);
}

// ---- ranked alternatives (qv_nbest.hip) ------------------------------------------------------------------------------
extern "C" int qv_nbest_results_ctx(qv_engine *eng, int32_t k_ctx, int32_t batch, int32_t k, int32_t flags, qv_nbest_info *info_host,
                                    qv_nbest_entry *entries_host) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(ctx_batch_args(eng, "qv_nbest_results_ctx", k_ctx, batch,
                          k >= 1 && k <= QV_NBEST_MAX && !(flags & ~QV_NBEST_TEXT_RUNNERS) && info_host && entries_host,
                          "bad context, null argument, empty batch, k outside 1..QV_NBEST_MAX or unknown flags"));
    return qv_nbest_results(eng, k_ctx, batch, k, flags, info_host, entries_host);
}

extern "C" int qv_nbest_select(qv_engine *eng, const double *final_host, const float *loss_host, const int32_t *n_host, int32_t rows,
                               int32_t pitch, int32_t k, int32_t *index_host, int32_t *count_host, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!final_host || !loss_host || !n_host || !index_host || !count_host || rows < 1 || pitch < 1 || pitch > QV_CAND_CAP || k < 1 ||
        k > QV_NBEST_MAX) {
        qv_set_error(eng, "qv_nbest_select: null argument, no rows, pitch outside 1..2048 or k outside 1..QV_NBEST_MAX");
        return QV_ERR_ARG;
    }
    QvCtx &c = eng->ctx[eng->cur_ctx];
    if (rows > c.work.max_batch) { qv_set_error(eng, "qv_nbest_select: rows exceed engine capacity"); return QV_ERR_CAPACITY; }
    for (int r = 0; r < rows; ++r)
        if (n_host[r] < 0 || n_host[r] > pitch) { qv_set_error(eng, "qv_nbest_select: n_host[r] outside 0..pitch"); return QV_ERR_ARG; }
    QV_ORDERED(eng, stream);
    return qv_nbest_select_rows(eng, c, final_host, loss_host, n_host, rows, pitch, k, index_host, count_host, (hipStream_t)stream);
}

// ---- recitation correction (qv_correct.hip) --------------------------------------------------------------------------
static bool correct_args_ok(const qv_engine *eng, int rows, int flags, const qv_correct_info *info_host, const uint8_t *ops_host,
                            int ops_pitch, const qv_correct_word *words_host, int words_pitch) {
    return rows >= 1 && !(flags & ~QV_CORRECT_PREFIX) && info_host && (!ops_host || ops_pitch >= QV_CORRECT_MAX_REF + eng->max_q) &&
           (!words_host || words_pitch >= QV_CORRECT_MAX_WORDS);
}

extern "C" int qv_correct(qv_engine *eng, const uint8_t *pred_codes_host, const int32_t *pred_off_host, const uint8_t *ref_codes_host,
                          const int32_t *ref_off_host, int32_t rows, int32_t flags, qv_correct_info *info_host, uint8_t *ops_host,
                          int32_t ops_pitch, qv_correct_word *words_host, int32_t words_pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!pred_codes_host || !pred_off_host || !ref_codes_host || !ref_off_host ||
        !correct_args_ok(eng, rows, flags, info_host, ops_host, ops_pitch, words_host, words_pitch)) {
        qv_set_error(eng, "qv_correct: null argument, no rows, unknown flags or a pitch below its cap");
        return QV_ERR_ARG;
    }
    QvCtx &c = eng->ctx[eng->cur_ctx];
    if (rows > c.work.max_batch) { qv_set_error(eng, "qv_correct: rows exceed engine capacity"); return QV_ERR_CAPACITY; }
    for (int r = 0; r < rows; ++r) {
        const int64_t np = (int64_t)pred_off_host[r + 1] - pred_off_host[r], nr = (int64_t)ref_off_host[r + 1] - ref_off_host[r];
        if (pred_off_host[r] < 0 || ref_off_host[r] < 0 || np < 0 || nr < 0 || np > QV_CORRECT_MAX_RAW || nr > QV_CORRECT_MAX_RAW) {
            qv_set_error(eng, "qv_correct: bad offsets or a text of more than QV_CORRECT_MAX_RAW codes");
            return QV_ERR_ARG;
        }
    }
    QV_ORDERED(eng, stream);
    return qv_correct_rows(eng, c, pred_codes_host, pred_off_host, ref_codes_host, ref_off_host, rows, flags, info_host, ops_host,
                           ops_pitch, words_host, words_pitch, (hipStream_t)stream);
}

extern "C" int qv_correct_results_ctx(qv_engine *eng, int32_t k_ctx, int32_t batch, int32_t flags, qv_correct_info *info_host,
                                      uint8_t *ops_host, int32_t ops_pitch, qv_correct_word *words_host, int32_t words_pitch) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(ctx_batch_args(eng, "qv_correct_results_ctx", k_ctx, batch,
                          correct_args_ok(eng, batch, flags, info_host, ops_host, ops_pitch, words_host, words_pitch),
                          "bad context, null argument, empty batch, unknown flags or a pitch below its cap"));
    return qv_correct_results(eng, k_ctx, batch, flags, info_host, ops_host, ops_pitch, words_host, words_pitch);
}

// ---- transcription with confidence (qv_transcribe.hip) ---------------------------------------------------------------
extern "C" int qv_transcribe(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch, int32_t t_max,
                             qv_transcript_info *info_host, int32_t *ids_host, float *logp_host, int16_t *first_host,
                             int16_t *last_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!lp || !t_host || !info_host || !ids_host || batch < 1 || t_max < 1 || pitch < t_max) {
        qv_set_error(eng, "qv_transcribe: null argument, empty batch, t_max < 1 or pitch < t_max");
        return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    return qv_transcribe_rows(eng, eng->ctx[eng->cur_ctx], lp, t_host, batch, t_max, info_host, ids_host, logp_host, first_host,
                              last_host, pitch, (hipStream_t)stream);
}

extern "C" int qv_transcribe_batch(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch, int64_t n_max,
                                   qv_transcript_info *info_host, int32_t *ids_host, float *logp_host, int16_t *first_host,
                                   int16_t *last_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    if (!audio_dev || !lengths_host || !info_host || !ids_host || batch < 1) {
        qv_set_error(eng, "qv_transcribe_batch: null argument or empty batch");
        return QV_ERR_ARG;
    }
    int t_max;
    QV_TRY(batch_in_capacity(eng, "qv_transcribe_batch: ", lengths_host, batch, &t_max));
    if (t_max < 1 || pitch < t_max) { qv_set_error(eng, "qv_transcribe_batch: pitch < qv_frames_for_samples(longest row)"); return QV_ERR_ARG; }
    QV_ORDERED(eng, stream);
    QvCtx *c;
    std::vector<int32_t> t_out;
    QV_TRY(forward_into_ws(eng, audio_dev, lengths_host, batch, n_max, t_max, (hipStream_t)stream, &c, t_out));
    return qv_transcribe_rows(eng, *c, c->logprobs_ws, t_out.data(), batch, t_max, info_host, ids_host, logp_host, first_host, last_host,
                              pitch, (hipStream_t)stream);
}

// ---- verse-constrained beam search (qv_beam.hip, qv_trie_host.h) ----------------------------------------------------
extern "C" int qv_trie_stats(const char *tables_path, int32_t max_span, int32_t *nodes, int32_t *ends, int32_t *max_depth,
                             int32_t *max_children) {
    if (!tables_path || max_span < 1 || max_span > QV_TRIE_MAX_SPAN) { qv_set_error(nullptr, "qv_trie_stats: null path or max_span outside 1..6"); return QV_ERR_ARG; }
    HostTables h;
    std::string err;
    if (int rc = qv_read_host_tables(tables_path, h, err)) { qv_set_error(nullptr, err); return rc; }
    QvTrie t;
    if (int rc = qv_trie_build(h.n_verses, h.tok_off.p, h.tok_off.n, h.tok.p, h.tok.n, max_span, t, err)) {
        qv_set_error(nullptr, err);
        return rc == QV_TRIE_BAD_ARG ? QV_ERR_ARG : QV_ERR_IO;
    }
    if (nodes) *nodes = (int32_t)t.n_nodes();
    if (ends) *ends = (int32_t)t.ends.size();
    if (max_depth) *max_depth = t.max_depth;
    if (max_children) *max_children = t.max_children;
    return QV_OK;
}

extern "C" int qv_trie_node_tokens(qv_engine *eng, int32_t max_span, int32_t node, int32_t *ids_out, int32_t cap, int32_t *n_out) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!ids_out || !n_out || cap < 0) { qv_set_error(eng, "qv_trie_node_tokens: null argument or cap < 0"); return QV_ERR_ARG; }
    return qv_beam_node_tokens(eng, max_span, node, ids_out, cap, n_out);
}

// the argument rules the two beam entry points share (everything but the log-probs and their frame counts)
static int beam_args(qv_engine *eng, const char *who, int32_t batch, int32_t max_span, int32_t beam, int32_t k, const void *info_host,
                     const void *entries_host, const int32_t *ids_host, int32_t pitch, int32_t t_max) {
    if (!info_host || !entries_host || batch < 1 || max_span < 1 || max_span > QV_TRIE_MAX_SPAN || beam < 1 || beam > QV_BEAM_MAX || k < 1 ||
        k > beam || (ids_host && pitch < t_max)) {
        qv_set_error(eng, std::string(who) + ": null argument, empty batch, max_span outside 1..6, beam outside 1..QV_BEAM_MAX, k outside 1..beam or pitch < t_max");
        return QV_ERR_ARG;
    }
    return QV_OK;
}

extern "C" int qv_beam_decode(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch, int32_t t_max, int32_t max_span,
                              int32_t beam, int32_t k, qv_beam_info *info_host, qv_beam_entry *entries_host, int32_t *ids_host,
                              int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!lp || !t_host || t_max < 1) { qv_set_error(eng, "qv_beam_decode: null argument or t_max < 1"); return QV_ERR_ARG; }
    QV_TRY(beam_args(eng, "qv_beam_decode", batch, max_span, beam, k, info_host, entries_host, ids_host, pitch, t_max));
    QV_ORDERED(eng, stream);
    return qv_beam_rows(eng, eng->ctx[eng->cur_ctx], lp, t_host, batch, t_max, max_span, beam, k, info_host, entries_host, ids_host, pitch,
                        (hipStream_t)stream);
}

extern "C" int qv_beam_batch(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch, int64_t n_max,
                             int32_t max_span, int32_t beam, int32_t k, qv_beam_info *info_host, qv_beam_entry *entries_host,
                             int32_t *ids_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    if (!audio_dev || !lengths_host || batch < 1) { qv_set_error(eng, "qv_beam_batch: null argument or empty batch"); return QV_ERR_ARG; }
    int t_max;
    QV_TRY(batch_in_capacity(eng, "qv_beam_batch: ", lengths_host, batch, &t_max));
    if (t_max < 1) { qv_set_error(eng, "qv_beam_batch: no frames"); return QV_ERR_ARG; }
    QV_TRY(beam_args(eng, "qv_beam_batch", batch, max_span, beam, k, info_host, entries_host, ids_host, pitch, t_max));
    QV_ORDERED(eng, stream);
    QvCtx *c;
    std::vector<int32_t> t_out;
    QV_TRY(forward_into_ws(eng, audio_dev, lengths_host, batch, n_max, t_max, (hipStream_t)stream, &c, t_out));
    return qv_beam_rows(eng, *c, c->logprobs_ws, t_out.data(), batch, t_max, max_span, beam, k, info_host, entries_host, ids_host, pitch,
                        (hipStream_t)stream);
}

// ---- exhaustive CTC scan (qv_scan.hip, qv_scan_plan.h) --------------------------------------------------------------
extern "C" int qv_scan_stats(const char *tables_path, int32_t t_frames, int32_t max_span, const uint32_t *surah_mask4, int32_t *n_feasible,
                             int32_t *n_recursions, int64_t *state_steps) {
    if (!tables_path || t_frames < 0 || t_frames > 2 * QV_SCAN_MAX_L + 2 || max_span < 1 || max_span > QV_SCAN_MAX_SPAN || qv_scan_mask_empty(surah_mask4)) {
        qv_set_error(nullptr, "qv_scan_stats: null path, t_frames outside 0..768, max_span outside 1..6 or a mask that selects nothing");
        return QV_ERR_ARG;
    }
    HostTables h;
    std::string err;
    if (int rc = qv_read_host_tables(tables_path, h, err)) { qv_set_error(nullptr, err); return rc; }
    QvScanView v;
    v.n_verses = h.n_verses;
    v.tok_off = h.tok_off.p; v.n_tok_off = h.tok_off.n;
    v.pfx = h.tok_pfx.data(); v.n_pfx = h.tok_pfx.size();
    v.surah = h.h_surah.data(); v.n_surah = h.h_surah.size();
    QvScanPlan p;
    int rc = qv_scan_view_check(v, err);
    if (!rc) rc = qv_scan_plan_make(v, t_frames, max_span, surah_mask4, p, err);
    if (rc) { qv_set_error(nullptr, err); return rc == QV_SCAN_BAD_ARG ? QV_ERR_ARG : QV_ERR_IO; }
    if (n_feasible) *n_feasible = p.n_feasible;
    if (n_recursions) *n_recursions = (int32_t)p.rec.size();
    if (state_steps) *state_steps = p.state_steps;
    return QV_OK;
}

// the argument rules the two scan entry points share (everything but the log-probs and their frame counts)
static int scan_args(qv_engine *eng, const char *who, int32_t batch, int32_t max_span, int32_t k, const uint32_t *mask_host,
                     const void *info_host, const void *entries_host) {
    bool bad = !info_host || !entries_host || batch < 1 || max_span < 1 || max_span > QV_SCAN_MAX_SPAN || k < 1 || k > QV_SCAN_MAX;
    for (int b = 0; !bad && mask_host && b < batch; ++b) bad = qv_scan_mask_empty(mask_host + (size_t)b * 4);
    if (bad) {
        qv_set_error(eng, std::string(who) + ": null argument, empty batch, max_span outside 1..6, k outside 1..QV_SCAN_MAX or a surah mask that selects nothing");
        return QV_ERR_ARG;
    }
    return QV_OK;
}

extern "C" int qv_scan_logprobs(qv_engine *eng, const float *lp, const int32_t *t_host, int32_t batch, int32_t t_max, int32_t max_span,
                                double span_penalty, int32_t k, const uint32_t *surah_mask_host, qv_scan_info *info_host,
                                qv_scan_entry *entries_host, float *loss_out_dev, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!lp || !t_host || t_max < 1) { qv_set_error(eng, "qv_scan_logprobs: null argument or t_max < 1"); return QV_ERR_ARG; }
    QV_TRY(scan_args(eng, "qv_scan_logprobs", batch, max_span, k, surah_mask_host, info_host, entries_host));
    QV_ORDERED(eng, stream);
    return qv_scan_rows(eng, eng->ctx[eng->cur_ctx], lp, t_host, batch, t_max, max_span, span_penalty, k, surah_mask_host, info_host,
                        entries_host, loss_out_dev, (hipStream_t)stream);
}

extern "C" int qv_scan_batch(qv_engine *eng, const float *audio_dev, const int64_t *lengths_host, int32_t batch, int64_t n_max,
                             int32_t max_span, double span_penalty, int32_t k, const uint32_t *surah_mask_host, qv_scan_info *info_host,
                             qv_scan_entry *entries_host, float *loss_out_dev, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    if (!audio_dev || !lengths_host || batch < 1) { qv_set_error(eng, "qv_scan_batch: null argument or empty batch"); return QV_ERR_ARG; }
    int t_max;
    QV_TRY(batch_in_capacity(eng, "qv_scan_batch: ", lengths_host, batch, &t_max));
    if (t_max < 1) { qv_set_error(eng, "qv_scan_batch: no frames"); return QV_ERR_ARG; }
    QV_TRY(scan_args(eng, "qv_scan_batch", batch, max_span, k, surah_mask_host, info_host, entries_host));
    QV_ORDERED(eng, stream);
    QvCtx *c;
    std::vector<int32_t> t_out;
    QV_TRY(forward_into_ws(eng, audio_dev, lengths_host, batch, n_max, t_max, (hipStream_t)stream, &c, t_out));
    return qv_scan_rows(eng, *c, c->logprobs_ws, t_out.data(), batch, t_max, max_span, span_penalty, k, surah_mask_host, info_host,
                        entries_host, loss_out_dev, (hipStream_t)stream);
}

extern "C" int qv_scan_kernel_times(qv_engine *eng, float *ms2_host) {
    QV_SERIALISE(eng);
    if (!eng || !ms2_host) return QV_ERR_ARG;
    if (!eng->profile_stages || qv_scan_times(eng, ms2_host)) { qv_set_error(eng, "qv_scan_kernel_times: no profiled scan (qv_profile_stages first)"); return QV_ERR_ARG; }
    return QV_OK;
}

// ---- recordings of any length (qv_long.hip, qv_long_plan.h) ---------------------------------------------------------
extern "C" int qv_long_plan(int64_t n_samples, int32_t max_samples, int32_t window_samples, int32_t margin_frames, int32_t *n_windows,
                            int32_t *t_total, int32_t *kw, int32_t *m) {
    QvLongPlan p;
    const int rc = qv_long_plan_make(n_samples, max_samples, window_samples, margin_frames, &p);
    if (rc) return rc;   // QV_ERR_ARG, or QV_ERR_CAPACITY above QV_LONG_MAX_FRAMES
    if (n_windows) *n_windows = p.n_windows;
    if (t_total) *t_total = p.t_total;
    if (kw) *kw = p.kw;
    if (m) *m = p.m;
    return QV_OK;
}

extern "C" int qv_transcribe_long(qv_engine *eng, const float *audio_dev, int64_t audio_pitch, const int64_t *lengths_host, int32_t rows,
                                  int32_t window_samples, int32_t margin_frames, qv_long_info *info_host, int32_t *ids_host,
                                  float *logp_host, int32_t *first_host, int32_t *last_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    if (!audio_dev || !lengths_host || !info_host || !ids_host || rows < 1 || audio_pitch < 1) {
        qv_set_error(eng, "qv_transcribe_long: null argument, no rows or audio_pitch < 1");
        return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    QvCtx *c;
    QV_TRY(claim_logprobs_ws(eng, &c));
    // (qv_long_run checks everything that can refuse the call before its first launch)
    return qv_long_run(eng, *c, audio_dev, audio_pitch, nullptr, 0, lengths_host, rows, window_samples, margin_frames, info_host,
                       ids_host, logp_host, first_host, last_host, pitch, (hipStream_t)stream);
}

extern "C" int qv_transcribe_windows(qv_engine *eng, const float *logprobs_dev, int32_t t_max, const int64_t *n_samples_host, int32_t rows,
                                     int32_t window_samples, int32_t margin_frames, qv_long_info *info_host, int32_t *ids_host,
                                     float *logp_host, int32_t *first_host, int32_t *last_host, int32_t pitch, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!logprobs_dev || !n_samples_host || !info_host || !ids_host || rows < 1 || t_max < 1) {
        qv_set_error(eng, "qv_transcribe_windows: null argument, no rows or t_max < 1");
        return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    return qv_long_run(eng, eng->ctx[eng->cur_ctx], nullptr, 0, logprobs_dev, t_max, n_samples_host, rows, window_samples, margin_frames,
                       info_host, ids_host, logp_host, first_host, last_host, pitch, (hipStream_t)stream);
}

// ---- word and verse timings for recordings of any length (qv_align_long.hip) ----------------------------------------
extern "C" int qv_align_long(qv_engine *eng, const float *audio_dev, int64_t audio_pitch, const int64_t *lengths_host, int32_t rows,
                             int32_t window_samples, int32_t margin_frames, const uint16_t *targets_host, const int32_t *lens_host,
                             qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host, float *logp_host, int32_t pitch,
                             void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    QV_TRY(need_model(eng));
    if (!audio_dev || !lengths_host || !lens_host || !info_host || !first_host || !last_host || !logp_host || rows < 1 || audio_pitch < 1) {
        qv_set_error(eng, "qv_align_long: null argument, no rows or audio_pitch < 1");
        return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    QvCtx *c;
    QV_TRY(claim_logprobs_ws(eng, &c));
    return qv_align_long_run(eng, *c, audio_dev, audio_pitch, nullptr, 0, lengths_host, rows, window_samples, margin_frames,
                             targets_host, lens_host, info_host, first_host, last_host, logp_host, pitch, (hipStream_t)stream);
}

extern "C" int qv_align_windows(qv_engine *eng, const float *logprobs_dev, int32_t t_max, const int64_t *n_samples_host, int32_t rows,
                                int32_t window_samples, int32_t margin_frames, const uint16_t *targets_host, const int32_t *lens_host,
                                qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host, float *logp_host, int32_t pitch,
                                void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!logprobs_dev || !n_samples_host || !lens_host || !info_host || !first_host || !last_host || !logp_host || rows < 1 || t_max < 1) {
        qv_set_error(eng, "qv_align_windows: null argument, no rows or t_max < 1");
        return QV_ERR_ARG;
    }
    QV_ORDERED(eng, stream);
    return qv_align_long_run(eng, eng->ctx[eng->cur_ctx], nullptr, 0, logprobs_dev, t_max, n_samples_host, rows, window_samples,
                             margin_frames, targets_host, lens_host, info_host, first_host, last_host, logp_host, pitch, (hipStream_t)stream);
}

extern "C" int qv_long_kernel_times(qv_engine *eng, float *ms3_host) {
    QV_SERIALISE(eng);
    if (!eng || !ms3_host) return QV_ERR_ARG;
    if (!eng->profile_stages || !eng->long_ws.m.dev) { qv_set_error(eng, "qv_long_kernel_times: no profiled long call (qv_profile_stages first)"); return QV_ERR_ARG; }
    memcpy(ms3_host, eng->long_ws.kernel_ms, sizeof(float) * 3);
    return QV_OK;
}

extern "C" int qv_align_long_kernel_times(qv_engine *eng, float *ms2_host) {
    QV_SERIALISE(eng);
    if (!eng || !ms2_host) return QV_ERR_ARG;
    if (!eng->profile_stages || !eng->align_long_ws.big) { qv_set_error(eng, "qv_align_long_kernel_times: no profiled long alignment (qv_profile_stages first)"); return QV_ERR_ARG; }
    memcpy(ms2_host, eng->align_long_ws.kernel_ms, sizeof(float) * 2);
    return QV_OK;
}

extern "C" int qv_debug_forward_tap(qv_engine *eng, int32_t what, int32_t layer, float *out_dev, void *stream) {
    QV_SERIALISE(eng);
    if (!eng) return QV_ERR_ARG;
    if (!eng->model) { qv_set_error(eng, "engine created without a model"); return QV_ERR_NO_MODEL; }
    QV_ORDERED(eng, stream);
    return qv_model_tap(eng, eng->model, eng->cur_ctx, what, layer, out_dev, (hipStream_t)stream);
}

// ---- measurement hooks -------------------------------------------------------------------
extern "C" int qv_profile_gemm(qv_engine *eng, int32_t enable) {
    if (!eng) return QV_ERR_ARG;
    qv_gemm_prof_enable(enable != 0);
    return QV_OK;
}

extern "C" int qv_profile_gemm_read(qv_engine *eng, double *ms21, double *flops21, int32_t *launches21) {
    if (!eng || !ms21 || !flops21 || !launches21) return QV_ERR_ARG;
    int n[21];
    qv_gemm_prof_collect(ms21, flops21, n);
    for (int i = 0; i < 21; ++i) launches21[i] = n[i];
    return QV_OK;
}

extern "C" int qv_profile_replay_kernel(qv_engine *eng, int32_t which, char *name_out, int32_t name_cap) {
    QV_SERIALISE(eng);
    if (!eng || !name_out || name_cap < 8) return QV_ERR_ARG;
    if (!eng->model) { qv_set_error(eng, "engine created without a model"); return QV_ERR_NO_MODEL; }
    return qv_model_replay_kernel(eng, eng->model, eng->cur_ctx, which, name_out, name_cap);
}

extern "C" int qv_weights_info(qv_engine *eng, char *out, int32_t cap) {
    QV_SERIALISE(eng);
    if (!eng || !out || cap < 16) return QV_ERR_ARG;
    if (!eng->model) { snprintf(out, (size_t)cap, "no acoustic model (post-logits stages only)"); return QV_OK; }
    qv_model_weights_info(eng->model, out, cap);
    return QV_OK;
}

extern "C" int qv_debug_attention_variant(int32_t mode) {
    if (mode < -1 || mode > 5) return QV_ERR_ARG;
    qv_attention_set_variant(mode);
    return QV_OK;
}

extern "C" int qv_debug_kernel_variant(int32_t which, int32_t mode) {
    if (which < 0 || which >= QV_KV_COUNT || mode < -1 || mode > 15) return QV_ERR_ARG;
    qv_kernel_variant_set(which, mode);
    return QV_OK;
}

extern "C" int qv_debug_sub01_plan(int64_t n_samples, int32_t batch, int32_t *frames_out, int32_t *run_tiles_out) {
    if (n_samples < 400 || batch < 1 || !frames_out) return QV_ERR_ARG;
    qv_model_frame_counts(n_samples, frames_out);
    if (run_tiles_out) *run_tiles_out = qv_sub01_run_tiles(batch, frames_out[2], qv_switches_now());
    return QV_OK;
}

extern "C" int qv_debug_sub35_plan(int64_t n_samples, int32_t batch, int32_t *run_frames_out) {
    if (n_samples < 400 || batch < 1 || !run_frames_out) return QV_ERR_ARG;
    int32_t fr[4];
    qv_model_frame_counts(n_samples, fr);
    *run_frames_out = qv_sub35_run_frames(batch, fr[3], qv_switches_now());
    return QV_OK;
}

extern "C" int qv_debug_forward_graph_stats(qv_engine *eng, int64_t *replays, int64_t *captures) {
    QV_SERIALISE(eng);
    if (!eng || !eng->model || !replays || !captures) return QV_ERR_ARG;
    qv_model_graph_stats(eng->model, replays, captures);
    return QV_OK;
}

extern "C" int64_t qv_debug_forward_graph_failures(qv_engine *eng) {
    QV_SERIALISE(eng);
    return (eng && eng->model) ? qv_model_graph_failures(eng->model) : -1;
}

extern "C" int qv_debug_gemm_tiles(int32_t mode) {
    if (mode < -1 || mode > 2) return QV_ERR_ARG;
    qv_gemm_set_t256(mode);
    return QV_OK;
}

extern "C" int qv_debug_gemm_tile_height(int32_t mode) {
    if (mode < -1 || mode > 3) return QV_ERR_ARG;
    qv_gemm_set_bm(mode);
    return QV_OK;
}

extern "C" int qv_debug_gemm_pipeline(int32_t ld, int32_t nst, int32_t narrow) {
    const int ids[3] = {QV_SW_GEMM_LD, QV_SW_GEMM_NST, QV_SW_GEMM_NARROW}, modes[3] = {ld, nst, narrow};
    for (int i = 0; i < 3; ++i)
        if (modes[i] < -1 || modes[i] > QV_SWITCH_TABLE[ids[i]].hi) return QV_ERR_ARG;   // (nothing is set when one is out of range)
    for (int i = 0; i < 3; ++i) qv_switch_set(ids[i], modes[i]);
    return QV_OK;
}

extern "C" int qv_profile_replay_gemm(qv_engine *eng, int32_t which, int32_t iters, double *avg_us, double *flops_per_launch,
                                      void *stream) {
    QV_SERIALISE(eng);
    if (!eng || !avg_us || !flops_per_launch) return QV_ERR_ARG;
    if (!eng->model) { qv_set_error(eng, "engine created without a model"); return QV_ERR_NO_MODEL; }
    return qv_model_replay_gemm(eng, eng->model, eng->cur_ctx, which, iters, avg_us, flops_per_launch, (hipStream_t)stream);
}
