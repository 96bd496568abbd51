// qv_common.h -- internal declarations shared by the translation units of libqverse.so.
// gfx950 only; no compatibility layers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qverse.h"
#include "qv_limits.h"   // QV_NSYM, QV_OTHER, QV_MAX_SPAN, QV_MAX_VW, qv_tmpl_w
#include "qv_long_plan.h"
#include "qv_switches.h"

#define QV_CAND_CAP 2048
#define QV_RUNNER_CAP 128
#define QV_RAW_CAP 4096     // raw (pre-collapse) transcript code units per utterance

#define QV_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            qv_set_error(eng, std::string(#expr) + ": " + hipGetErrorString(e_));            \
            return QV_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

struct qv_engine;
void qv_set_error(qv_engine *e, const std::string &msg);

// Device memory that lives as long as its owner (`allocs`: qv_engine::allocs or QvModel::allocs, freed by qv_destroy), at
// least 16 bytes each: `count` elements copied from the host / `count` zeroed elements.
template <typename T>
int qv_dev_upload(qv_engine *eng, std::vector<void *> &allocs, const T *host, size_t count, const T **dev) {
    void *p = nullptr;
    QV_HIP(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    allocs.push_back(p);
    if (count) QV_HIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
    *dev = (const T *)p;
    return QV_OK;
}
template <typename T>
int qv_dev_zeroed(qv_engine *eng, std::vector<void *> &allocs, size_t count, T **dev) {
    void *p = nullptr;
    QV_HIP(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
    QV_HIP(hipMemset(p, 0, std::max<size_t>(count * sizeof(T), 16)));
    allocs.push_back(p);
    *dev = (T *)p;
    return QV_OK;
}

// ------------------------------------------------------------------ static tables -----
// Device-resident verse database (built once at qv_create from qverse_tables.bin).
struct QvTables {
    int n_verses, n_surah, n_tri, n_text;  // n_text = 2N + #nobsm
    // verse identity
    const uint8_t *surah;        // [N]
    const uint16_t *ayah;        // [N]
    const int32_t *surah_start;  // [n_surah+1]
    const int32_t *surah_len;    // [n_surah]
    // clean texts laid out back to back WITH one ' ' between consecutive verses, so every
    // span text (first.no_bsm||clean + ' ' + rest.clean) is one contiguous slice
    const uint8_t *clean;        // codes
    const uint32_t *clean_off;   // [N]
    const uint16_t *clean_len;   // [N]
    const uint16_t *nobsm_len;   // [N] 0 = none; text = last nobsm_len codes of clean[v]
    // the same texts once more for the prefix-shared span pass (k_spans2): verse v is the block [clean8_off[v],
    // clean8_off[v + 1]) = one ' ', its codes, then filler codes (0xFF: match nothing, leave the LCS recurrence alone) up
    // to a multiple of 8 -- every ayah END falls on the end of an 8-code chunk.  Built at qv_create.
    const uint8_t *clean8;
    const uint32_t *clean8_off;  // [N+1], multiples of 8
    const uint8_t *alt;
    const uint32_t *alt_off;     // [N]
    const uint16_t *alt_len;     // [N]
    const uint16_t *nw[3];       // word counts clean / alt / nobsm
    const int32_t *nobsm_rank;   // [N] index among verses that have a no_bsm text, -1 otherwise
    // word ends of the clean texts: wend[wend_off[v] + k] = chars of the first k+1 words joined
    const uint32_t *wend_off;    // [N+1]
    const uint16_t *wend;
    const int32_t *len_order;    // [N] verse indices, longest clean text first (lanes of a wave get similar lengths)
    // per-text bit-parallel match masks (pattern = the verse text): text id = variant*N + v for
    // variant 0/1, 2N + nobsm_rank for variant 2.  layout [QV_NSYM][words]
    const uint64_t *pmv;
    const uint32_t *pmv_off;     // [n_text] offset in u64 units
    // trigram index (forward form)
    const uint32_t *tri_keys;    // [n_tri] sorted packed trigrams
    const double *tri_idf;       // [n_tri]
    const uint32_t *vtri_off;    // [N+1]
    const uint16_t *vtri;        // sorted trigram ids per verse
    // ... and the inverted form: verses of each trigram in ascending order; tri_slice[id*5 + w] is
    // where the verses of quarter w of the verse range start (w = 4: end of the list)
    const uint16_t *tri_post;
    const uint16_t *tri_map;     // [2^18] packed trigram (6 bits per code) -> id, 0xFFFF = not in the index
    const uint32_t *tri_slice;   // [n_tri * 5]
    // CTC token table: key = v*6 + (span-1)
    const uint32_t *tok_off;     // [N*6+1]
    const uint16_t *tok;
    // bit k-1 of tok_pfx[v]: the ids of (v, span k) are a PREFIX of the ids of (v, span k+1) (SentencePiece
    // segments word by word, so a span's ids normally extend the shorter span's; not so where the first ayah
    // loses its bismillah in a span).  Built at qv_create; lets k_ctc share one alpha recursion between them.
    const uint8_t *tok_pfx;      // [N]
    // vocabulary pieces: normalised code strings
    const uint32_t *piece_off;   // [1026]
    const uint8_t *piece_codes;
};

// ------------------------------------------------------------------ per-batch state ---
struct QvUtt {           // one per utterance, device memory (SoA would not buy anything here)
    int32_t t_frames;
    int32_t n_tok;
    int32_t q_len, qs_len, q_words;
    int32_t flags;
    int32_t n_cand1;       // pass-1 iteration list length
    int32_t full_scan;     // 1 if pass 1 iterates all verses
    int32_t best1_idx;     // best single verse (index) after pass 1
    double best1_score;
    int32_t n_runners;
    int32_t n_surah20;
    int32_t surah20[20];
    int32_t base_start, base_span;   // -1 = none
    double base_score;
    int32_t use_ctc;
    int32_t n_cand;
    int32_t n_lead;        // candidates that run an alpha recursion (k_candidates' plan for k_ctc)
    int32_t win;           // winning candidate index or -1
    float win_norm;
    // match_verse with a continuation hint and without the trigram restriction (qv_match_verse;
    // the hot path leaves both at 0): up to 3 verses get a bonus and a suffix-prefix score
    int32_t force_full;
    int32_t hint_n;
    int32_t hint_v[3];
    double hint_bonus[3];
    double hint_sp[3];
};

struct QvWork {
    int max_batch, t_cap;
    QvUtt *utt;              // [B]
    int16_t *frame_ids;      // [B][t_cap]
    int32_t *greedy;         // [B][t_cap]
    uint8_t *q;              // [B][max_q]   (max_q: the window of the kernel set the engine runs -- eng->match->max_q)
    uint8_t *qs;             // [B][max_q] spaceless
    uint64_t *pm;            // [B][2][QV_NSYM][max_q / 64]  (0: q, 1: spaceless q)
    int32_t *cand1;          // [B][N]
    int16_t *lcsf;           // [B][N][3] full-string LCS(transcript, text) (clean, alt, nobsm)
    double *fs;              // [B][N][3] fragment scores (clean, alt, nobsm)
    int16_t *lcs_p3;         // [B][N]   pass 3: LCS(spaceless transcript, clean text) (k_lcs_full mode 1)
    uint32_t *frag_list;     // [B * N * 3] texts whose fragment score needs the window scan: utterance << 15 | verse << 2 | variant
    int32_t *frag_ctr;       // [4]: expensive entries (front of frag_list), work-stealing cursor of k_frag, cheap entries (back of the list)
    int frag_cap;            // entries frag_list holds
    double *search_sc;       // [B][N]   search score (max over clean/alt)
    int32_t *runner_idx;     // [B][QV_RUNNER_CAP]
    double *runner_score;    // [B][QV_RUNNER_CAP]
    int32_t *top_search;     // [B][QV_RUNNER_CAP]
    double *top_search_sc;
    int32_t *top_p3;         // [B][QV_RUNNER_CAP]
    double *top_p3_sc;
    double *span_part_score; // [B][QV_SPAN_BLOCKS]
    uint64_t *span_part_key; // [B][QV_SPAN_BLOCKS]
    int32_t *cand_start;     // [B][QV_CAND_CAP]
    int32_t *cand_span;      // [B][QV_CAND_CAP]
    double *cand_score;      // [B][QV_CAND_CAP]
    int16_t *cand_lead;      // [B][QV_CAND_CAP] list of the leaders' candidate indices (first n_lead entries)
    int16_t *cand_memb;      // [B][QV_CAND_CAP][QV_MAX_SPAN] per leader: candidate index of its (start, span k) prefix, -1 = none
    float *cand_loss;        // [B][QV_CAND_CAP]
    double *cand_final;      // [B][QV_CAND_CAP]
    qv_result *results;      // [B]
    int32_t *packed;         // [B][4]
    int32_t *fail_list;      // [B] compacted gate-fail utterance indices
    int32_t *n_fail;         // [1]
};

#define QV_SPAN_BLOCKS 64

struct QvKnobs {
    int top_text, top_span_refs, max_span;
    double threshold, text_weight, span_penalty;
    int skip_unused;
};

// verse tracker workspace (qv_tracker_match): QV_TRACK_CAP texts per launch
#define QV_TRACK_CAP 256
#define QV_TRACK_BLOCKS 32   // >= ceil(n_verses / 256) partial maxima per text
#define QV_RESAMPLE_ROWS 1024   // rows per qv_upfirdn_batch / qv_mixdown_batch call
#define QV_RESAMPLE_SLOTS 16    // calls whose row tables may be in flight on a stream at once
struct QvTrack {
    uint8_t *q;          // [CAP * max_q] codes of the slice's texts, back to back
    int32_t *meta;       // [CAP][4] q_len, n_words, bonus verse, offset in q
    double *part_s;      // [CAP][QV_TRACK_BLOCKS]
    uint64_t *part_k;    // [CAP][QV_TRACK_BLOCKS] verse * 2 + (no_bsm variant matched)
    qv_track_match *out; // [CAP]
};

// A device buffer and the pinned host buffer that mirrors its first host_bytes: what the row-wise features send their inputs
// up and fetch their records back through in ONE copy (qv_rows.h: qv_mirror_alloc / qv_mirror_free and the helpers around
// them).  A context's mirrors belong to QvCtx::mirrors; the engine-level one of the long transcription to QvLongWs.
struct QvMirror {
    unsigned char *dev, *host;
    size_t dev_bytes, host_bytes;
};
// Per-context workspace of a feature that sends the rows' frame counts up and gets one record per row back (transcription,
// beam search), allocated by the first call that uses it (m.dev == nullptr: not yet): the frame counts in the first t_bytes
// of the mirror, the records of max_batch rows behind them.
struct QvRowWs {
    QvMirror m;
    size_t t_bytes;
};

// forced alignment (qv_align.hip).  One row of the launch plan: which token list (offset into the token buffer the kernel
// is given: the table's, or the staged explicit targets), how many tokens, how many frames.
#define QV_ALIGN_PITCH 384   // entries per row of the device-side outputs (>= QV_ALIGN_MAX_TOKENS)
struct QvAlignRow { int32_t tok_off, L, T, flags, start, span; };
// per-context alignment workspace, allocated by the first alignment call on that context (bp == nullptr: not yet).
// Outputs are one record per row -- qv_align_info, then logp / first / last / ids with QV_ALIGN_PITCH entries each -- so a
// batch comes back in ONE copy into a pinned buffer, from where the host scatters it into the caller's arrays; plan and
// explicit targets travel the same way in the other direction.  One mirror holds it all: out, plan and targets at the front
// of the device buffer and in the pinned one, the back-pointers behind them on the device alone.
#define QV_ALIGN_ROW_BYTES (sizeof(qv_align_info) + QV_ALIGN_PITCH * (sizeof(float) + 3 * sizeof(int16_t)))
struct QvAlignWs {
    uint32_t *bp;            // [B][t_cap][64] back-pointers: two bits per state, a lane's NS states in one word
    unsigned char *out;      // [B][QV_ALIGN_ROW_BYTES]
    QvAlignRow *plan;        // [B], followed in the same allocation by
    uint16_t *targets;       // [B * QV_ALIGN_PITCH] explicit targets of qv_align, back to back
    unsigned char *out_host; // pinned mirror of out
    unsigned char *in_host;  // pinned mirror of plan + targets
};
struct QvCtx;
int qv_align_explicit(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, const uint16_t *targets_host,
                      const int32_t *lens_host, qv_align_info *info_host, int16_t *first_host, int16_t *last_host,
                      float *logp_host, int pitch, hipStream_t stream);
int qv_align_results(qv_engine *eng, int k, int batch, qv_align_info *info_host, uint16_t *ids_host, int16_t *first_host,
                     int16_t *last_host, float *logp_host, int pitch);

// ranked alternatives (qv_nbest.hip).  One record per row -- qv_nbest_info, then QV_NBEST_MAX entries -- so a batch comes
// back in ONE copy into a pinned buffer, from where the host hands the first k entries of every row to the caller.
#define QV_NBEST_ROW_BYTES (sizeof(qv_nbest_info) + QV_NBEST_MAX * sizeof(qv_nbest_entry))
#define QV_NBEST_SEL_PITCH (QV_NBEST_MAX + 1)   // qv_nbest_select's device output per row: the count, then the indices
// per-context n-best workspace, allocated by the first n-best call on that context (out == nullptr: not yet); the staging
// arrays of the explicit form by the first qv_nbest_select (sel_final == nullptr: not yet)
struct QvNbestWs {
    unsigned char *out;       // [B][QV_NBEST_ROW_BYTES]
    unsigned char *out_host;  // pinned mirror of out (qv_nbest_select's indices come back through it as well)
    double *sel_final;        // [B][QV_CAND_CAP], followed in the same allocation by
    float *sel_loss;          // [B][QV_CAND_CAP]
    int32_t *sel_n;           // [B]
    int32_t *sel_idx;         // [B][QV_NBEST_SEL_PITCH]
};
int qv_nbest_results(qv_engine *eng, int k_ctx, int batch, int k, int flags, qv_nbest_info *info_host, qv_nbest_entry *entries_host);
int qv_nbest_select_rows(qv_engine *eng, QvCtx &c, const double *final_host, const float *loss_host, const int32_t *n_host, int rows,
                         int pitch, int k, int32_t *index_host, int32_t *count_host, hipStream_t stream);

// recitation correction (qv_correct.hip).  One record per row -- qv_correct_info, the op codes, the words -- so a batch comes
// back in ONE copy into the pinned mirror; the explicit entry's codes and offsets go up through the same mirror.  Allocated
// by the first correction call on the context (m.dev == nullptr: not yet); the back-pointers sit behind the mirrored part,
// on the device alone, for min(max_batch, QV_CORRECT_ROUND) rows.
#define QV_CORRECT_ROUND 64
struct QvCorrectWs {
    QvMirror m;
    size_t row_bytes, ops_cap;   // one record; op codes it holds (QV_CORRECT_MAX_REF + the engine's window)
    size_t in_off, bp_off;       // staged input (offsets, then codes) and back-pointers within the device buffer
    size_t bp_row_words;         // uint32 words of back-pointers per row
};
int qv_correct_rows(qv_engine *eng, QvCtx &c, const uint8_t *pred_codes, const int32_t *pred_off, const uint8_t *ref_codes,
                    const int32_t *ref_off, int rows, int flags, qv_correct_info *info_host, uint8_t *ops_host, int ops_pitch,
                    qv_correct_word *words_host, int words_pitch, hipStream_t stream);
int qv_correct_results(qv_engine *eng, int k_ctx, int batch, int flags, qv_correct_info *info_host, uint8_t *ops_host, int ops_pitch,
                       qv_correct_word *words_host, int words_pitch);

// transcription with confidence (qv_transcribe.hip).  One record per row -- qv_transcript_info, then ids / logp / first /
// last with P = t_max rounded up to even entries each -- so a batch comes back in ONE copy into the pinned mirror (QvRowWs).
int qv_transcribe_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max,
                       qv_transcript_info *info_host, int32_t *ids_host, float *logp_host, int16_t *first_host, int16_t *last_host,
                       int pitch, hipStream_t stream);

// verse-constrained beam search (qv_beam.hip; the trie: qv_trie_host.h).  One record per row -- qv_beam_info, then QV_BEAM_MAX
// (node, total, pb, pnb) entries -- so a batch comes back in ONE copy into the pinned mirror (QvRowWs).  The trie of the span
// last asked for belongs to the engine (QvBeamState, nullptr until a call needs it).
struct QvBeamState;
struct QvTrie;
void qv_beam_free(qv_engine *eng);
int qv_beam_trie(qv_engine *eng, int max_span, const QvTrie **out);
int qv_beam_node_tokens(qv_engine *eng, int max_span, int node, int32_t *ids_out, int cap, int32_t *n_out);
int qv_beam_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, int max_span, int W, int k,
                 qv_beam_info *info_host, qv_beam_entry *entries_host, int32_t *ids_host, int pitch, hipStream_t stream);

// exhaustive CTC scan (qv_scan.hip; the launch plan: qv_scan_plan.h).  One record per row -- qv_scan_info, then QV_SCAN_MAX
// entries -- comes back in ONE copy into the pinned mirror (QvCtx::scan); the host copies of the table parts the plans are
// made from belong to the engine (QvScanState, nullptr until a call needs it).
struct QvScanState;
void qv_scan_free(qv_engine *eng);
int qv_scan_times(qv_engine *eng, float *ms2);   // qv_profile_stages: the last call's time in k_ctc_scan and k_scan_select
int qv_scan_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, int max_span, double penalty,
                 int k, const uint32_t *mask_host, qv_scan_info *info_host, qv_scan_entry *entries_host, float *loss_out_dev,
                 hipStream_t stream);

// recordings of any length (qv_long.hip; the cutting rule: qv_long_plan.h).  One workspace per engine, allocated or grown by
// the first call that needs it and freed by qv_destroy: the mirror's device buffer holds the plan tables (tab_bytes,
// rec_bytes), the records (out_bytes), then fid (fid_bytes) and m; its pinned buffer mirrors tables and records; `batch` is
// the [max_batch, window_samples] batch the windows of a round are gathered into (engines with a model).
struct QvLongWs {
    QvMirror m;
    float *batch;
    size_t batch_cap;   // floats
    size_t tab_bytes, rec_bytes, out_bytes, fid_bytes;
    float kernel_ms[3];   // qv_profile_stages: the last call's time in k_long_gather, k_long_frames, k_long_collapse
};
void qv_long_free(QvLongWs &w);
int qv_long_run(qv_engine *eng, QvCtx &c, const float *audio, int64_t audio_pitch, const float *lp_in, int t_max_in,
                const int64_t *n_host, int rows, int window_samples, int margin_frames, qv_long_info *info_host, int32_t *ids_host,
                float *logp_host, int32_t *first_host, int32_t *last_host, int pitch, hipStream_t stream);
// What qv_long_run is made of, for the other caller of the windowed forward (qv_align_long.hip).  One window of the call, in
// the flattened recording-then-window order (device plan table):
struct QvLongWin {
    int64_t src_off;   // first sample of the window in the caller's audio (elements)
    int64_t dst;       // index of the window's first OWNED frame in the fid / m arrays
    int32_t len;       // samples to copy; the rest of the row is zero
    int32_t lp_win;    // the window's row in the log-prob tensor the round's kernel reads
    int32_t j0;        // local index of the first owned frame
    int32_t count;     // owned frames
};
struct QvLongRec { int32_t t_frames, n_windows; };
struct QvLongTimer;
// a call after qv_long_check (nothing allocated or launched yet) and qv_long_tables (tables in the long workspace, uploaded)
struct QvLongCall {
    std::vector<QvLongPlan> plans;   // per recording
    std::vector<int64_t> fwd_len;    // per window: the length the forward is given (audio calls)
    size_t n_win;
    int t_top, kw, wn, P;            // most frames of a recording; frames and samples of a full window; t_top rounded up to 4
    const QvLongWin *tab_d;
    const QvLongRec *rec_d;
};
// every check of a long call that does not concern its outputs; `who` is the entry point's name in the error text
int qv_long_check(qv_engine *eng, const char *who, QvCtx &c, const float *audio, int64_t audio_pitch, int t_max_in,
                  const int64_t *n_host, int rows, int window_samples, int margin_frames, QvLongCall &call);
int qv_long_tables(qv_engine *eng, QvCtx &c, bool audio, int64_t audio_pitch, int rows, QvLongCall &call, hipStream_t stream);
// the rounds: per_round(lp, t_max, k0, nb) enqueues what reads windows k0 .. k0 + nb - 1 of the table out of lp f32[*, t_max, 1025]
// (the context's log-prob workspace, reused by the next round, or the caller's tensor) -- in stream order, nothing waits
int qv_long_rounds(qv_engine *eng, QvCtx &c, const QvLongCall &call, const float *audio, int64_t audio_pitch, const float *lp_in,
                   int t_max_in, hipStream_t stream, QvLongTimer *tm,
                   const std::function<int(const float *lp, int t_max, size_t k0, int nb)> &per_round);

// word and verse timings of recordings of any length (qv_align_long.hip; the byte formula: qv_align_long_plan.h).  One
// workspace per engine, grown on need and freed by qv_destroy: `big` holds the kept log-prob rows of every recording and
// behind them the back-pointers; the mirror carries the plan rows, the windows' destinations and the targets up and the
// records back.
struct QvAlignLongWs {
    QvMirror m;
    unsigned char *big;
    size_t big_bytes;
    float kernel_ms[3];   // qv_profile_stages: the last call's time in k_long_keep and k_align_long (the third is unused)
};
void qv_align_long_free(QvAlignLongWs &w);
int qv_align_long_run(qv_engine *eng, QvCtx &c, const float *audio, int64_t audio_pitch, const float *lp_in, int t_max_in,
                      const int64_t *n_host, int rows, int window_samples, int margin_frames, const uint16_t *targets_host,
                      const int32_t *lens_host, qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host,
                      float *logp_host, int pitch, hipStream_t stream);

// The matching window is a compile-time constant of the kernels that touch the transcript (buffer pitches, LDS arrays, the
// word counts the LCS core is instantiated for).  Those kernels -- and only those -- are compiled once per window
// (qv_match_body.inc through qv_match.hip and qv_match_wide.hip); each compilation defines one QvMatchSet.  qv_create stores
// a pointer to the set that matches qv_config.max_transcript, and the post-logits launchers launch through it.
struct QvMatchSet {
    int max_q;                // the window, 1024 or 2048
    int decode_threads;       // k_decode's block size
    int frag_blocks;          // k_frag's grid
    size_t trigram_lds;       // k_trigram's dynamic LDS behind its n_verses scores
    void (*k_decode)(QvTables, QvWork, const float *, int, const int32_t *);
    void (*k_prepare_codes)(QvWork, int);
    void (*k_trigram)(QvTables, QvWork), (*k_frag)(QvTables, QvWork);
    void (*k_lcs_full)(QvTables, QvWork, int), (*k_hint_sp)(QvTables, QvWork, int);
    void (*k_spans)(QvTables, QvWork, QvKnobs), (*k_spans2)(QvTables, QvWork, QvKnobs);
    void (*k_track)(QvTables, QvTrack);
    // The one window-independent kernel a set may carry: its own long-target CTC rerank, k_ctc<true, VAR> per wave program
    // VAR, or nullptr = the one of qv_postlogits.hip.  The wide set has its own (qv_ctc_body.inc says why).
    void (*k_ctc_long[2])(QvTables, QvWork, QvKnobs, const float *, int);
};
// (hidden: unmangled names that are no part of the library's exported C symbols)
extern const QvMatchSet qv_match_default __attribute__((visibility("hidden"))), qv_match_wide __attribute__((visibility("hidden")));

// post-logits launchers (qv_postlogits.hip); `c` is the execution context whose workspace and staging slots the call uses
int qv_post_tracker_match(qv_engine *eng, const uint8_t *codes_host, const int32_t *offsets_host,
                          const int32_t *n_words_host, const int32_t *bonus_host, int batch,
                          qv_track_match *out_host, hipStream_t stream);
int qv_post_run(qv_engine *eng, QvCtx &c, const float *logprobs_dev, int t_max, const int32_t *t_host, int batch,
                hipStream_t stream);
int qv_post_debug_retrieve(qv_engine *eng, QvCtx &c, const uint8_t *codes_host, int n, hipStream_t stream);
int qv_post_match_verse(qv_engine *eng, QvCtx &c, const uint8_t *codes_host, int n, int n_bonus, const int32_t *bonus_verse,
                        const double *bonus_value, int max_span, hipStream_t stream);
int qv_post_debug_ctc(qv_engine *eng, const float *lp, int T, const uint16_t *tg, const int32_t *lens, int n,
                      float *loss_host, hipStream_t stream);

// acoustic model (qv_model.hip)
struct QvModel;
int qv_model_create(qv_engine *eng, const qv_config *cfg, const QvSwitches &sw, QvModel **out);   // sw: qv_create's snapshot (taps, cross-check paths)
void qv_model_destroy(QvModel *m);
// `k` is the execution context whose activations (and forward graphs) the call works on
int qv_model_forward(qv_engine *eng, QvModel *m, int k, const float *audio_dev, const int64_t *len_host, int batch,
                     int64_t n_max, float *logprobs_dev, int t_max, int32_t *t_out_host, hipStream_t stream,
                     bool zero_pad_rows = false,    // true: rows t >= T[b] of logprobs_dev are zeroed (the public qv_forward)
                     bool may_graph = false);       // true: `stream` is one of the engine's own (capturable) context streams
int qv_model_tap(qv_engine *eng, QvModel *m, int k, int what, int layer, float *out_dev, hipStream_t stream);
// frames of a clip of n_samples after the log-mel front end and after each of the three stride-2 stages (the forward's own arithmetic)
void qv_model_frame_counts(int64_t n_samples, int32_t out[4]);
int qv_model_replay_gemm(qv_engine *eng, QvModel *m, int k, int which, int iters, double *avg_us, double *flops, hipStream_t s);
int qv_model_replay_kernel(qv_engine *eng, QvModel *m, int k, int which, char *name_out, int cap);

void qv_model_weights_info(const QvModel *m, char *out, int cap);
void qv_model_graph_stats(const QvModel *m, int64_t *replays, int64_t *captures);
int64_t qv_model_graph_failures(const QvModel *m);   // captures / instantiations that failed (the context then runs plain launches)
// records stage event `i` of context `c` on `s` when stage profiling is on (qv_capi.hip)
void qv_stage_mark(qv_engine *eng, QvCtx &c, int i, hipStream_t s);

// One execution context = everything a batch in flight owns; this struct is the only home of its post-logits state (the
// model keeps the activations of context k in QvModel::ctx_acts[k]).  Functions that work on a context are handed it.
// With n_ctx > 1, qv_predict_batch_async() round-robins the contexts, each on its own internal
// stream, so the latency-bound post-logits kernels of one batch run under the forward of the next.
#define QV_MAX_CTX 8
// Pinned staging buffers (frame counts here, the model's length table in QvActs) are written by the host
// and then read by an asynchronous H2D copy: each has QV_STAGE_SLOTS slots used in turn, and a slot is
// reused only after the event recorded behind its copy has completed -- back-to-back asynchronous calls
// on one context (n_contexts = 1 included) never overwrite lengths a queued copy has yet to read.
#define QV_STAGE_SLOTS 2
struct QvCtx {
    QvWork work = {};
    float *logprobs_ws = nullptr;        // [max_batch][t_cap][1025] log-prob workspace (engines with a model)
    int32_t *t_host_scratch = nullptr;   // [QV_STAGE_SLOTS][max_batch] pinned
    int32_t *t_dev = nullptr;            // [max_batch]
    hipStream_t stream = nullptr;        // n_ctx > 1: the context's own stream, with the events that fence a batch on it
    hipEvent_t in_ready = nullptr, done = nullptr;
    bool busy = false;
    int last_batch = 0, last_tmax = 0;   // shape of the last post-logits run on this context
    hipEvent_t t_copied[QV_STAGE_SLOTS] = {};
    bool t_pending[QV_STAGE_SLOTS] = {};
    int t_slot = 0;
    // stage timers (qv_profile_stages): start, forward done, decode done, build done, rerank done
    hipEvent_t stage_ev[5] = {};
    bool stage_valid = false;
    // the post-logits chain (k_decode .. k_result, 13 kernels) as ONE hipGraph launch, keyed by what the kernel
    // arguments depend on; captured the first time a key is seen on this context
    struct PostGraph { const float *lp; int batch, t_max, variants; hipGraphExec_t exec; } post_graph[4] = {};   // variants: the kernel variants in force (spans, CTC) and the engine's window
    bool post_graph_off = false;   // a capture / instantiate failed on this context: plain launches from then on
    int n_post_graph = 0;
    // forced alignment (qv_align_results_ctx): what the context's last batch was decoded from -- log-prob tensor (the
    // context's workspace or the caller's), its row pitch in frames, batch size, the stream the chain ran on -- and the
    // lazily allocated workspace.  al_lp == nullptr: nothing to align (no batch yet, or the workspace was reused).
    const float *al_lp = nullptr;
    int al_tmax = 0, al_batch = 0;
    hipStream_t al_stream = nullptr;
    // The mirrors of this context's lazily allocated feature workspaces.  This list OWNS them, both halves: qv_ctx_mirror
    // (qv_rows.h) appends, one loop in qv_destroy frees through qv_mirror_free; nothing of a mirror is in qv_engine::allocs.
    // The pointers the workspaces below keep into them are views.
    std::vector<QvMirror> mirrors;
    QvAlignWs align = {};
    // ranked alternatives (qv_nbest_results_ctx): the same batch, read from the candidate arrays of `work`
    QvNbestWs nbest = {};
    // recitation correction (qv_correct_results_ctx: the same batch, its transcript in `work`; qv_correct: explicit texts)
    QvCorrectWs correct = {};
    // transcription with confidence (qv_transcribe, qv_transcribe_batch): independent of the batch state above
    QvRowWs transcribe = {};
    // verse-constrained beam search (qv_beam_decode, qv_beam_batch): independent of the batch state as well
    QvRowWs beam = {};
    // exhaustive CTC scan (qv_scan_logprobs, qv_scan_batch): independent of the batch state too (layout: qv_scan_rows)
    QvMirror scan = {};
};

struct qv_engine {
    // every entry point that touches the engine takes this lock for the duration of the HOST call (entry points call
    // one another, hence recursive): calls from several host threads are serialised instead of corrupting the shared
    // host-side state (context rotation, staging slots); the device work they enqueue stays asynchronous
    std::recursive_mutex mu;
    // ... and consecutive calls that enqueue on DIFFERENT caller streams are ordered on the device as well (they share
    // a context's workspace): each such call waits for the event the previous one left behind (QvStreamOrder)
    hipEvent_t tail_ev = nullptr;
    hipStream_t tail_stream = nullptr;
    bool tail_valid = false;
    qv_config cfg;
    int max_q = QV_MAX_TRANSCRIPT;   // the matching window, 1024 or 2048
    const QvMatchSet *match = &qv_match_default;   // the matching kernels compiled for that window
    QvKnobs knobs;
    int device;
    std::string last_error;
    QvTables tab;                 // device pointers
    std::vector<void *> allocs;   // everything hipMalloc'ed for tables/work
    QvCtx ctx[QV_MAX_CTX];
    // cur_ctx: index of the context of the most recent asynchronous call (qv_last_context), written by
    // qv_predict_batch_async alone.  The entry points without a context argument act on ctx[cur_ctx].
    int n_ctx, cur_ctx, next_ctx;
    QvModel *model;
    // resampler filters already arranged per phase and resident in HBM (qv_upfirdn)
    struct Fir { int up; std::vector<float> taps; float *hflip_dev; int P; };
    std::vector<Fir> firs;
    unsigned char *resample_tab = nullptr;   // ring of row tables for qv_upfirdn_batch / qv_mixdown_batch
    unsigned resample_at = 0;
    QvTrack track;
    QvLongWs long_ws = {};
    QvAlignLongWs align_long_ws = {};
    QvBeamState *beam = nullptr;   // the trie of the beam search (qv_beam.hip), built by the first call that asks for it
    QvScanState *scan = nullptr;   // the scan's host copies of the token table's offsets and prefix flags (qv_scan.hip)
    bool profile_stages;
    // measurement hook (qv_profile_inject_logprobs): caller-owned log-probs the post-logits stages of
    // qv_predict_batch_async() read INSTEAD of the forward's own output (the forward still runs in full)
    const float *inject_lp;
    int inject_tmax, inject_batch;
    std::vector<int32_t> inject_t;
    // host copies of small table parts used by debug/entry code
    std::vector<uint8_t> h_surah;
    std::vector<uint16_t> h_ayah;
};
