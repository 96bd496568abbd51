/*
 * qverse.h -- C ABI of libqverse.so, the MI355X-native replacement for the numerics of
 * the reference's c2c-direct-mixed hot path (paths relative to yazinsai/offline-tarteel):
 *
 *   audio_signal f32[B,N] --qv_forward--> log-probs f32[B,T,1025]
 *        replaces  onnxruntime InferenceSession.run(None, {"audio_signal","length"})
 *                  experiments/c2c-direct-mixed/run.py:55-63, .../c2c-direct-mixed-tta/run.py:74-79
 *   log-probs --qv_decode_retrieve_rerank--> (surah, ayah, ayah_end, score, source)
 *        replaces  _greedy_decode        experiments/c2c-direct/run.py:187-204
 *                  _build_candidates     experiments/c2c-direct/run.py:251-311
 *                  QuranDB.match_verse / search  shared/quran_db.py:92-99,244-371
 *                  _ctc_rerank (torch F.ctc_loss) experiments/c2c-direct/run.py:314-380
 *                  decision logic        experiments/c2c-direct-mixed/run.py:96-133
 *   qv_predict_batch = both, back to back on one stream (what predict() does per file,
 *        experiments/c2c-direct-mixed/run.py:66-133, for a whole batch).
 *
 * Conventions
 *   - plain C, no torch types.  Pointers named *_dev are DEVICE pointers owned by the
 *     caller (e.g. PyTorch-ROCm tensors); the library never frees or retains them.
 *     Pointers named *_host are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Entry points
 *     enqueue work on it; only functions documented as synchronous wait for it.
 *   - every function returns 0 on success or a QV_ERR_* code; qv_last_error() gives text.
 *     The Python binding turns non-zero into an exception, so the runner's per-sample
 *     try/except (benchmark/runner.py:322-325) yields the reference's empty prediction.
 *   - one engine per process per GPU.  Host calls on one engine are serialised by the library (a
 *     per-engine lock held for the duration of each call), so calling from several threads is safe --
 *     the reference's TTA plugin runs its 0.9x / 1.1x passes from two threads
 *     (c2c-direct-mixed-tta/run.py:129-130) -- but gains nothing: batching the work into one call
 *     (what plugin.predict_tta does) or keeping batches in flight (qv_predict_batch_async) is the
 *     GPU-native form.  Results of a context must be fetched before that context is reused.
 *     The ASYNC protocol (qv_predict_batch_async -> qv_last_context -> qv_fetch_results_ctx) is one logical sequence:
 *     drive it from ONE thread per engine (or under the caller's own lock) -- another thread's call in between moves
 *     qv_last_context().  qv_last_error() returns a copy private to the calling thread.
 */
#ifndef QVERSE_H
#define QVERSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QV_VOCAB 1025
#define QV_BLANK 1024
#define QV_MAX_TRANSCRIPT 1024      /* normalised transcript chars handled on device: the default window */
#define QV_MAX_TRANSCRIPT_WIDE 2048 /* ... and the opt-in wide one (qv_config.max_transcript) */

enum {
    QV_OK = 0,
    QV_ERR_ARG = 1,        /* bad argument / unsupported knob */
    QV_ERR_IO = 2,         /* tables or weights file missing / malformed (FileNotFoundError) */
    QV_ERR_HIP = 3,        /* HIP runtime error */
    QV_ERR_CAPACITY = 4,   /* batch / length exceeds what the engine was created for */
    QV_ERR_NO_MODEL = 5    /* forward requested but engine has no weights */
};

enum { QV_SOURCE_NONE = 0, QV_SOURCE_TEXT = 1, QV_SOURCE_CTC = 2 };

/* flags in qv_result.flags */
enum {
    QV_FLAG_EMPTY_TRANSCRIPT = 1,   /* greedy decode produced nothing -> _empty("") */
    QV_FLAG_TRANSCRIPT_TRUNCATED = 2,/* more chars than the engine's window (qv_max_transcript): prediction withheld (surah 0) */
    QV_FLAG_USED_CTC = 4,           /* gate failed (base.score < threshold): rerank ran */
    QV_FLAG_CAND_OVERFLOW = 8       /* candidate list clipped at engine capacity */
};

typedef struct qv_engine qv_engine;

/* Arithmetic of the acoustic model.
 *   QV_PREC_FP16             f16 weights and GEMM operands, f32 accumulation / residual stream.
 *   QV_PREC_MIXED_INT4_INT8  storage formats of the reference's file with f16 arithmetic: block-128 int4 Linear weights and
 *                            per-channel int8 pointwise-conv weights, dequantised in the MFMA operand fetch (W4A16 / W8A16).
 *   QV_PREC_ORT_MIXED        the ARITHMETIC onnxruntime runs on the reference's file (experiments/c2c-direct-mixed/run.py:1-9):
 *                            MatMulNBits int4 on the Linear layers, and on EVERY Conv DynamicQuantizeLinear -> ConvInteger:
 *                            per-utterance uint8 activations (range from the tensor's own min / max), one symmetric int8
 *                            scale per weight tensor, int32 accumulation (i8 MFMA for the GEMM-shaped convolutions, exact
 *                            integer stencils for the depthwise / strided ones), float32 rescale.  csrc/qv_ort.h. */
enum { QV_PREC_FP16 = 0, QV_PREC_MIXED_INT4_INT8 = 1, QV_PREC_ORT_MIXED = 2 };

typedef struct {
    int32_t struct_size;        /* sizeof(qv_config), for forward compatibility */
    int32_t device;             /* HIP device ordinal */
    const char *tables_path;    /* qverse_tables.bin (tools/build_tables.py) */
    const char *weights_path;   /* flat weight file (tools/convert_weights.py) or NULL */
    uint64_t random_weights_seed; /* used when weights_path == NULL and with_model != 0 */
    int32_t with_model;         /* 0: post-logits stages only */
    int32_t precision;          /* QV_PREC_* */
    int32_t max_batch;          /* capacity: utterances per call */
    int32_t max_samples;        /* capacity: samples per utterance (480000 = 30 s); at most 976,000 (61 s):
                                   the CTC rerank holds 2L+1 <= T <= 768 states per candidate */
    /* CTC_DIRECT_* knobs, experiments/c2c-direct/run.py:62-74 (same defaults) */
    int32_t top_text;           /* CTC_DIRECT_TOP_TEXT        100 */
    int32_t top_span_refs;      /* CTC_DIRECT_TOP_SPAN_REFS    80 */
    int32_t max_span;           /* CTC_DIRECT_MAX_SPAN          6 (table limit 6) */
    double threshold;           /* CTC_DIRECT_THRESHOLD       0.80 */
    double text_weight;         /* CTC_DIRECT_TEXT_WEIGHT      0.0 (final = -norm_loss + weight * text score - penalty);
                                   any finite value, negative included, as c2c-direct/run.py:67 */
    double span_penalty;        /* CTC_DIRECT_SPAN_PENALTY     0.5 */
    int32_t skip_unused_passes; /* 1: skip search()/pass-3 when the gate passes (their output is
                                   unused by the mixed plugin); 0: literal */
    int32_t n_contexts;         /* 1..8 batches in flight (default 1).  With > 1,
                                   qv_predict_batch_async() rotates over that many execution
                                   contexts (own activations, workspace and internal stream), so
                                   the latency-bound decode/retrieval/CTC kernels of one batch run
                                   under the forward pass of the next.  Memory scales with it. */
    int32_t max_transcript;     /* matching window in normalised chars: 0 or 1024 (QV_MAX_TRANSCRIPT, the default) or
                                   2048 (QV_MAX_TRANSCRIPT_WIDE: a second set of matching kernels with a 32-word
                                   pattern; about 12 KB more state per utterance and context).  Anything else is
                                   QV_ERR_ARG.  Appended after the first published layout: qv_create() accepts a
                                   struct_size that ends with n_contexts and reads this field as 0. */
} qv_config;

/* One prediction; mirrors the dict of experiments/c2c-direct-mixed/run.py:126-133. */
typedef struct {
    int32_t surah, ayah, ayah_end;  /* 0,0,0 = no match (_empty) */
    int32_t source;                 /* QV_SOURCE_* */
    double score;                   /* unrounded; the mixed plugin rounds to 4 dp, TTA does not */
    double base_score;              /* match_verse score (0 if none) */
    float ctc_norm_loss;            /* winner's loss / len when source == CTC */
    int32_t n_tokens;               /* greedy token count */
    int32_t n_chars;                /* normalised transcript length */
    int32_t n_candidates;           /* candidates scored by the rerank (0 if gate passed) */
    int32_t flags;                  /* QV_FLAG_* */
    int32_t t_frames;               /* encoder frames of this utterance */
} qv_result;

void qv_config_default(qv_config *cfg);
int qv_create(const qv_config *cfg, qv_engine **out);
void qv_destroy(qv_engine *e);
const char *qv_last_error(const qv_engine *e); /* e may be NULL: last create() error */
/* The engine's matching window: 1024 or 2048 normalised chars (qv_config.max_transcript); 0 for a NULL engine. */
int32_t qv_max_transcript(const qv_engine *e);

/* Encoder frames produced for n_samples of 16 kHz audio (three stride-2 stages over
 * floor(n/160)+1 mel frames). */
int32_t qv_frames_for_samples(int64_t n_samples);

/* Acoustic model.  audio_dev: f32[B, n_max] row-major, rows zero-padded past lengths_host[b].
 * logprobs_dev: f32[B, t_max, 1025] with t_max >= qv_frames_for_samples(max length); rows
 * t >= T[b] are ZEROED (onnxruntime hands the reference exactly [1, T, 1025], mixed/run.py:59-63: a padded batch tensor
 * never exposes uninitialised memory).  t_out_host[b] receives T[b] (computed on the host, no sync).
 * Isolation: the valid frames of row b are a function of that row's lengths_host[b] samples alone -- the same bits whatever
 * the other rows of the batch, or earlier batches on the engine, held, NaN / +-inf / samples whose spectrum overflows float32
 * included (tests/test_gpu_forward_isolation.py).  A row WITH non-finite samples keeps its frame count T[b] and its zeroed
 * rows t >= T[b]; its valid frames hold unspecified values, finite or not.  Such a row is outside the contract of every
 * post-logits entry point below ("valid frames hold no NaN"), qv_predict_batch and the other calls that run them on the
 * forward's output included: what they do with it is not defined. */
int qv_forward(qv_engine *e, const float *audio_dev, const int64_t *lengths_host, int32_t batch,
               int64_t n_max, float *logprobs_dev, int32_t t_max, int32_t *t_out_host, void *stream);

/* Post-logits stages on log-probs already in HBM.  t_host[b] = valid frames of row b.
 * results_host: qv_result[B]; greedy_ids_host (optional, may be NULL): i32[B, t_max] collapsed
 * token ids (-1 padded) for host-side transcript text.  SYNCHRONOUS: returns after the results
 * have been copied back (one stream sync at the end, none in between).
 * Rows t >= t_host[b] of logprobs_dev are NEVER READ, here, by qv_align and by the calls that go back to the tensor
 * (qv_align_results_ctx): they may hold anything, NaN included.  Valid frames hold no NaN. */
int qv_decode_retrieve_rerank(qv_engine *e, const float *logprobs_dev, const int32_t *t_host,
                              int32_t batch, int32_t t_max, qv_result *results_host,
                              int32_t *greedy_ids_host, void *stream);

/* Asynchronous variant: results stay in an engine-owned device buffer; fetch with
 * qv_fetch_results() after the stream (or an event) has completed. */
int qv_decode_retrieve_rerank_async(qv_engine *e, const float *logprobs_dev, const int32_t *t_host,
                                    int32_t batch, int32_t t_max, void *stream);
int qv_fetch_results(qv_engine *e, int32_t batch, int32_t t_max, qv_result *results_host,
                     int32_t *greedy_ids_host, void *stream);

/* forward + post-logits on the engine's own log-prob workspace.  SYNCHRONOUS like above. */
int qv_predict_batch(qv_engine *e, const float *audio_dev, const int64_t *lengths_host,
                     int32_t batch, int64_t n_max, qv_result *results_host,
                     int32_t *greedy_ids_host, void *stream);
int qv_predict_batch_async(qv_engine *e, const float *audio_dev, const int64_t *lengths_host,
                           int32_t batch, int64_t n_max, void *stream);

/* Same, and returns the execution context the batch runs on in *ctx_out under the same lock hold -- what a caller
 * that may share the engine with other threads passes to qv_wait_ctx / qv_fetch_results_ctx / qv_packed_results_ctx
 * (qv_last_context() after a separate call can already name another thread's batch). */
int qv_predict_batch_async_ctx(qv_engine *e, const float *audio_dev, const int64_t *lengths_host,
                               int32_t batch, int64_t n_max, void *stream, int32_t *ctx_out);

/* ---- a15: speed perturbation / sample-rate conversion ------------------------------------
 * The float32 polyphase FIR behind scipy.signal.resample_poly(x, up, down), which the reference's
 * TTA wrapper calls with (9, 10) and (11, 10) (experiments/c2c-direct-mixed-tta/run.py:60-71):
 *   y[m] = sum_j x[xi - (P-1) + j] * h[t + up * (P-1-j)],  xi = (m0+m)*down / up, t = (m0+m)*down % up,
 * P = ceil(n_taps / up), terms outside [0, n_in) skipped, accumulated IN THIS ORDER in float32
 * (no FMA), which is what scipy's upfirdn does -- results are bit-identical to it.
 * taps_host: n_taps float32 filter taps exactly as resample_poly hands them to upfirdn (designed,
 * scaled by `up`, zero-padded in front/behind); m0 = first kept output sample (n_pre_remove).
 * x_dev [n_in], y_dev [n_out] device pointers.  Asynchronous on `stream`. */
int qv_upfirdn(qv_engine *e, const float *x_dev, int64_t n_in, const float *taps_host, int32_t n_taps,
               int32_t up, int32_t down, int64_t m0, int64_t n_out, float *y_dev, void *stream);

/* The same FIR over a BATCH of rows in one launch: output row r = resample of source row src_rows_host[r] (NULL: row r) of
 * x_dev [.., x_pitch], n_in_host[r] samples long; y_dev row r [y_pitch] receives ceil(n_in * up / down) samples followed by
 * zeros up to y_pitch -- the engine's zero-padded [B, N] input layout, so the result can go straight into qv_predict_batch.
 * Used by the TTA wrapper (all 0.9x or all 1.1x copies of a batch's gated clips: one launch instead of one per clip) and by
 * the device ingest of non-16 kHz files (160/441, 1/3: offline-tarteel_amd/audio.py load_audio_device; reference
 * shared/audio.py:8-18).  Per sample the arithmetic is qv_upfirdn's, term for term.  rows <= 1024.  Asynchronous on
 * `stream`; the host arrays may be released on return. */
int qv_upfirdn_batch(qv_engine *e, const float *x_dev, int64_t x_pitch, const int32_t *src_rows_host, const int64_t *n_in_host,
                     int32_t rows, const float *taps_host, int32_t n_taps, int32_t up, int32_t down, int64_t m0,
                     float *y_dev, int64_t y_pitch, void *stream);
/* Interleaved multi-channel rows [frames][channels] (float32) -> mono rows: the float32 mean over the channel axis, one
 * division of the frame's sum by the channel count, i.e. numpy's x.reshape(-1, ch).mean(axis=1) -- the reference's mix-down
 * (shared/audio.py:13-15) -- bit for bit.  The sum is taken in numpy's order: left to right from +0 below 8 channels; from 8
 * up, eight running sums r[k] = x[k], r[k] += x[8 i + k] over the whole groups of eight, joined as
 * ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the channels % 8 tail one by one.  A frame of -0.0 gives +0.0, as
 * numpy's does.  1 <= channels <= 64, rows <= 1024; samples behind a row's n_frames are left as they are. */
int qv_mixdown_batch(qv_engine *e, const float *x_dev, int64_t x_pitch, const int64_t *n_frames_host, int32_t rows,
                     int32_t channels, float *y_dev, int64_t y_pitch, void *stream);

/* ---- batches in flight (n_contexts > 1) -------------------------------------------------
 * qv_predict_batch_async() then only ORDERS ITS INPUTS on `stream` (the audio must stay unchanged
 * until the call's results have been joined) and runs on the context's internal stream; a call
 * blocks the host only when the context it is about to reuse is still busy.  Results are joined
 * per context: */
int32_t qv_context_count(const qv_engine *e);      /* may be lower than qv_config.n_contexts, see below */
/* How many of FOUR fresh HIP streams -- what a four-context engine is about to create -- the runtime runs side by side on
 * this device: 4, 2 or 1 (0 = probe failed).  Four one-wave spin kernels on four streams, elapsed time over spin time
 * (~1 ms, cached per process).  The runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and reads the
 * variable ONCE, when HIP initialises; streams sharing a queue serialise.  Measured: with 8 queues 7 fresh streams run
 * concurrently (4 once RCCL holds its own), on the default 4 queues only 3.  qv_create() calls this when n_contexts >= 4
 * and falls back to 3 contexts -- the best measured setting on the default queues -- unless all four ran concurrently, so
 * that a host which touched HIP before exporting GPU_MAX_HW_QUEUES=8 loses ~2 % instead of ~14 %. */
int32_t qv_probe_concurrent_streams(void);
/* dev tool: the probe's raw figure (elapsed time / spin time) for n_streams fresh streams, not cached */
double qv_debug_probe_rounds(int32_t n_streams);
int32_t qv_last_context(const qv_engine *e);     /* context used by the most recent async call */
/* Host-side join: blocks the calling thread until context `ctx`'s last batch has finished (no-op for an idle
 * context).  A device-side join (qv_packed_results_ctx on a stream) parks a wait on an OLDER batch in that stream's
 * hardware queue; when the runtime maps another stream onto the same queue, that stream's work is stuck behind it. */
int qv_wait_ctx(qv_engine *e, int32_t ctx);
/* makes `stream` wait for that context's batch, then returns its packed i32[B,4] rows */
const int32_t *qv_packed_results_ctx(qv_engine *e, int32_t ctx, void *stream);
/* host copy of that context's results (SYNCHRONOUS) */
int qv_fetch_results_ctx(qv_engine *e, int32_t ctx, int32_t batch, int32_t t_max, qv_result *results_host,
                         int32_t *greedy_ids_host);

/* ---- streaming row: the verse tracker's matching step -------------------------------------
 * Replaces VerseTracker._find_best_match (shared/verse_tracker.py:67-101) with _score_verse
 * (:41-65) inlined: for each of `batch` accumulated texts, the scan of all 6,236 verses (clean
 * text, and the bismillah-stripped variant where the verse has one) of
 *     raw = blend(ratio(text, first min(n_text, n_verse) words of the verse), ratio(text, verse))
 *           [+ 0.15 for the verse after the last emission]
 * and the first maximum in verse order.  Texts arrive as alphabet codes (0 = ' ', 63 = a
 * character outside the verse alphabet), concatenated, text b = codes[offsets[b] ..
 * offsets[b+1]); n_words_host[b] = number of whitespace-separated words of text b;
 * bonus_verse_host[b] = global index of the verse that gets the continuation bonus
 * (QuranDB.get_next_verse of the last emission, shared/quran_db.py:81-90) or -1.
 * out_host[b].verse = -1 when no verse scores above 0.0; the minimum-emit-score and
 * minimum-word-count gates of the caller are NOT applied here.  Texts longer than the
 * engine's window (qv_max_transcript() codes) are refused (QV_ERR_CAPACITY), as they are by
 * qv_match_verse and qv_debug_retrieve.  SYNCHRONOUS on `stream`. */
typedef struct qv_track_match {
    int32_t verse;     /* global verse index, -1 = none */
    int32_t surah, ayah;
    int32_t variant;   /* 0 = text_clean matched, 2 = text_clean_no_bsm */
    int32_t n_words;   /* words of the matched text (what _emit trims by, verse_tracker.py:110-114) */
    int32_t reserved;
    double score;
} qv_track_match;
int qv_tracker_match(qv_engine *e, const uint8_t *codes_host, const int32_t *offsets_host,
                     const int32_t *n_words_host, const int32_t *bonus_verse_host, int32_t batch,
                     qv_track_match *out_host, void *stream);

/* QuranDB.match_verse(text, max_span, hint) WITHOUT the trigram restriction (shared/quran_db.py:
 * 244-371 with use_trigram_index=False), as StreamingPipeline.run_on_full_transcript calls it
 * (shared/streaming.py:86): pass 1 scores every verse (fragment scores of text_clean /
 * text_clean_alt / text_clean_no_bsm; for the <= 3 verses of the continuation hint also
 * _suffix_prefix_score, :188-208, plus their bonus, _continuation_bonuses :121-146), pass 2 every
 * window of 2..max_span ayat of the surahs of the top 20.  codes_host: the NORMALISED text as
 * alphabet codes; bonus_verse / bonus_value: n_bonus (0..3) global verse indices and their
 * bonuses; max_span in [2, 8].  Outputs the winner (first verse index, number of ayat, score);
 * the caller applies the threshold.  SYNCHRONOUS on `stream`.  Uses the workspace of the most
 * recently used execution context (waits for batches in flight first): fetch the results of an
 * asynchronous batch before calling it. */
int qv_match_verse(qv_engine *e, const uint8_t *codes_host, int32_t n_codes, int32_t n_bonus,
                   const int32_t *bonus_verse, const double *bonus_value, int32_t max_span,
                   int32_t *start, int32_t *span, double *score, void *stream);

/* ---- word timings: CTC forced alignment ----------------------------------------------------
 * Which frames did every token of a target occupy?  A Viterbi pass (max in place of the CTC loss's log-sum-exp) over
 * the blank-extended target, float32 in natural-log units: v[0][0] = lp[0][blank], v[0][1] = lp[0][tgt[0]], every other
 * state -1e30;  v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is odd, s > 1 and tgt[s/2] != tgt[s/2-1])
 * + lp[t][ext[s]].  Ties go to the smaller step (stay, then s-1, then s-2).  The path ends in state S-1 = 2L if
 * v[T-1][S-1] >= v[T-1][S-2], else in S-2.  The only float operation per state and frame is that one add, so `score`
 * (the value of the final state) is reproducible bit for bit.  Per token i: first[i] / last[i] = first and last frame
 * (inclusive) spent in state 2i+1, logp[i] = the float32 sum of lp[t][tgt[i]] over those frames divided by their count.
 * A frame is 1,280 samples (0.08 s).  Rows with a flag set hold -1 in first / last / ids, 0 in logp and score; so do the
 * entries past a row's n_tokens.  Output rows are `pitch` entries apart, pitch >= QV_ALIGN_MAX_TOKENS (else QV_ERR_ARG).
 * The back-pointer workspace (max_batch * t_cap * 256 bytes per context) is allocated by the first alignment call that
 * uses the context.  Both calls are SYNCHRONOUS. */
#define QV_ALIGN_MAX_TOKENS 383          /* 2L+1 <= 767 states, the CTC rerank's own bound */
enum { QV_ALIGN_NO_TARGET = 1,           /* L == 0 / the row has no prediction (surah 0) */
       QV_ALIGN_TOO_LONG = 2,            /* L > QV_ALIGN_MAX_TOKENS or 2L+1 above the engine's state capacity (384 states for an
                                            engine of at most 384 frames, 30 s; 768 above) */
       QV_ALIGN_INFEASIBLE = 4 };        /* T < L + number of adjacent equal tokens: no path */
typedef struct { int32_t n_tokens, flags, t_frames, start_verse, span, reserved; float score, reserved_f; } qv_align_info;

/* explicit targets (any ids 0..1023), like qv_debug_ctc_loss but batched: row b aligns targets[off[b]..] (off = running sum
 * of lens_host) to log-prob row b of logprobs_dev f32[batch, t_max, 1025], t_host[b] valid frames.  start_verse = -1,
 * span = 0.  t_max above the engine's frame capacity or batch above max_batch: QV_ERR_CAPACITY. */
int qv_align(qv_engine *e, const float *logprobs_dev, const int32_t *t_host, int32_t batch, int32_t t_max,
             const uint16_t *targets_host, const int32_t *lens_host,
             qv_align_info *info_host, int16_t *first_host, int16_t *last_host, float *logp_host, int32_t pitch, void *stream);
/* the winners of context ctx's last batch against the log-probs that batch was decoded from: each row's (start verse, span)
 * is read from the device-side result (QV_SOURCE_TEXT and QV_SOURCE_CTC winners alike), its token list is the table's --
 * what the CTC rerank scores; ids_host receives it.  After qv_predict_batch[_async[_ctx]] the log-probs are the context's
 * own workspace; after qv_decode_retrieve_rerank[_async] they are the CALLER's tensor, which must still be alive and
 * unchanged.  Like qv_fetch_results_ctx it must be called before the context is reused (the next batch on it, or
 * qv_match_verse / qv_debug_retrieve, which run on the current context's workspace); it waits for the batch itself. */
int qv_align_results_ctx(qv_engine *e, int32_t ctx, int32_t batch, qv_align_info *info_host, uint16_t *ids_host,
                         int16_t *first_host, int16_t *last_host, float *logp_host, int32_t pitch);

/* ---- ranked alternatives (n-best) -------------------------------------------------------------
 * The reference's predict() also returns "candidates": the head of the rerank's ranked list, or [best] when the gate
 * passed (experiments/c2c-direct/run.py:424-435).  The list is selected on the device from what the batch left in HBM;
 * one fixed-size record per row comes back in one copy.
 *   QV_SOURCE_CTC rows   the stable top k of the row's reranked candidates with a finite loss, by final_score descending,
 *                        ties to the smaller candidate index (run.py:378-379; IEEE > and == on doubles, so -0.0 and +0.0
 *                        tie).  Entry 0 is the winner qv_result reports: same candidate, ctc_norm_loss with the same bits.
 *   QV_SOURCE_TEXT rows  (the gate passed, or the rerank ran and no candidate was feasible) entry 0 is the text match with
 *                        score = text_score = qv_result.base_score.  With QV_NBEST_TEXT_RUNNERS match_verse's runners-up
 *                        follow in its order: single verses, scores unrounded; the runner that IS a single-verse base is
 *                        not repeated.  Without the flag the list is [best], as in the reference.
 *   rows without a prediction (empty or withheld transcript, surah 0): n_entries = 0.
 * Entries past n_entries are zeroed. */
#define QV_NBEST_MAX 32
enum { QV_NBEST_TEXT_RUNNERS = 1 };
typedef struct {
    int32_t surah, ayah, ayah_end, start_verse, span;
    int32_t cand_index;   /* index in the reranked candidate list; -1 for text entries */
    int32_t source;       /* QV_SOURCE_CTC | QV_SOURCE_TEXT */
    int32_t n_tokens;     /* CTC target length; 0 for text entries */
    double  score;        /* CTC: final_score (run.py:376); TEXT: the text score */
    double  text_score;
    float   ctc_loss, ctc_norm_loss;
} qv_nbest_entry;
typedef struct { int32_t n_entries, n_ranked /* finite-loss candidates */, source, flags /* the row's QV_FLAG_* */; } qv_nbest_info;

/* The n-best lists of context ctx's last batch: info_host[batch], entries_host[batch][k], 1 <= k <= QV_NBEST_MAX; flags:
 * QV_NBEST_*.  SYNCHRONOUS.  Like qv_align_results_ctx it must be called before the context is reused (the next batch on
 * it, or qv_match_verse / qv_debug_retrieve, which run on the current context's workspace), and it waits for the batch
 * itself: on the context's own stream when the batch ran there, after a device-wide join when it ran on a caller stream.
 * Works after qv_predict_batch[_async[_ctx]] and after qv_decode_retrieve_rerank[_async], with either matching window.
 * The workspace (max_batch records of 1,808 bytes in device memory plus a pinned mirror) is allocated by the first call
 * that uses the context; one device-to-host copy per call.  Bad context, null pointer, batch < 1, a batch the context
 * does not hold, k outside 1..QV_NBEST_MAX or unknown flags: QV_ERR_ARG; batch above max_batch: QV_ERR_CAPACITY. */
int qv_nbest_results_ctx(qv_engine *e, int32_t ctx, int32_t batch, int32_t k, int32_t flags,
                         qv_nbest_info *info_host, qv_nbest_entry *entries_host);
/* The same selection on caller-supplied vectors: row r ranks the entries c < n_host[r] of final_host[r * pitch + c] whose
 * loss_host[r * pitch + c] is finite.  index_host[rows][k] receives the indices in rank order, -1 padded; count_host[rows]
 * how many.  rows <= max_batch (else QV_ERR_CAPACITY), 0 <= n_host[r] <= pitch <= 2048, 1 <= k <= QV_NBEST_MAX (else
 * QV_ERR_ARG).  NaN scores are never selected.  SYNCHRONOUS on `stream`; uses the current context's n-best workspace. */
int qv_nbest_select(qv_engine *e, const double *final_host, const float *loss_host, const int32_t *n_host,
                    int32_t rows, int32_t pitch, int32_t k, int32_t *index_host, int32_t *count_host, void *stream);

/* ---- recitation correction: word-level errors against the verse ------------------------------------
 * Which words did the reciter get wrong?  The reference answers with a Levenshtein alignment under a fixed tie rule
 * (shared/phoneme_aligner.py: align_phonemes) folded into words (web/frontend/src/lib/correction.ts: computeCorrection);
 * there it runs on phonemes, here on alphabet codes.  Every output is an integer.
 *   symbols     code 0 (space) is never a symbol, it only separates words.  pred / ref = the predicted / reference text with
 *               its spaces removed, m = |pred|, n = |ref|; word(r) = number of spaces in front of reference symbol r in the
 *               reference text; n_words = 1 + number of spaces in the reference text (runs of spaces in an explicit text make
 *               words without symbols).  Codes compare by plain equality: 63 is an ordinary symbol.
 *   DP          dp[i][0] = i, dp[0][j] = j;  sub = dp[i-1][j-1] + (ref[i-1] != pred[j-1]), del = dp[i-1][j] + 1,
 *               ins = dp[i][j-1] + 1, dp[i][j] = min of the three; the move is S if dp[i][j] == sub, else D if == del, else I
 *               (phoneme_aligner.py:75-89, ties in that order).
 *   backtrace   from (n, m) to (0, 0): at i == 0 the move is I, at j == 0 it is D; the list is then reversed.  One op code per
 *               alignment column: 0 match (S, equal), 1 substitution (S, unequal), 2 deletion (D), 3 insertion (I).  The
 *               position of a column = reference symbols consumed before it (phoneme_aligner.py:116-148).
 *   words       a column at position p belongs to word(p) if p < n, else to word(n - 1): trailing insertions go to the last
 *               word (correction.ts:60-78).  Per word: n_match, n_sub, n_del, n_ins, n_symbols = n_match + n_sub + n_del (the
 *               word's aligned symbols) and type = 0 without an error, 1 with any substitution, else the op code of its first
 *               error in alignment order (2 or 3).
 *   prefix      QV_CORRECT_PREFIX, for a recitation in progress (what computeCorrection's maxWordIndex approximates by hand):
 *               the backtrace starts at (i*, m), i* = the smallest i in 0..n that minimises dp[i][m]; reference symbols >= i*
 *               are not part of the alignment and words that own none of the aligned symbols report zeros (the word of symbol
 *               i* still receives the trailing insertions: position i* follows the rule above).  n_ref_used = i* (n without
 *               the flag), words_touched = words that own a symbol < i*, QV_CORRECT_LAST_WORD_OPEN = symbols i*-1 and i* belong
 *               to one word.
 *   per row     qv_correct_info; distance = dp[i*][m] = n_sub + n_del + n_ins, n_ops = alignment columns.  The reference's per
 *               and correct_rate are distance / n_ref_used and n_match / n_ref_used: left to the caller.
 *   row flags   QV_CORRECT_NO_TARGET: n == 0 or the row has no prediction; QV_CORRECT_NO_TRANSCRIPT: m == 0 (computeCorrection's
 *               empty return); QV_CORRECT_TOO_LONG: n > QV_CORRECT_MAX_REF, m > qv_max_transcript(e) or n_words >
 *               QV_CORRECT_MAX_WORDS.  A row that carries one of the three returns no ops and no words and every other info
 *               field 0.
 * The longest spaceless text of a (verse, span <= 6) in the shipped tables has 1,223 symbols and the wordiest 280 words
 * (tests/test_correct_host.py walks the tables); the longest single verse has 551 symbols.
 * Outputs: ops_host[row * ops_pitch + c] = op code of column c, 0xFF past n_ops, ops_pitch >= QV_CORRECT_MAX_REF +
 * qv_max_transcript(e); words_host[row * words_pitch + w], zeroed past n_words, words_pitch >= QV_CORRECT_MAX_WORDS.  Either
 * may be NULL.  Both calls are SYNCHRONOUS.  The workspace belongs to the execution context and is allocated by the first
 * call that uses it: per row of max_batch a record of 64 + (1280 + window) + 12 * 288 bytes in device memory and pinned,
 * 4,096 bytes of staged codes (explicit entry), and for min(max_batch, 64) rows the back-pointers -- 2 bits per DP cell,
 * (1280 + window + 1) diagonals of 81 words: 746,820 bytes per row with the default window, 1,078,596 with the wide one.
 * More than 64 rows run in rounds of 64 inside one call; one device-to-host copy per call. */
#define QV_CORRECT_MAX_REF 1280
#define QV_CORRECT_MAX_WORDS 288
#define QV_CORRECT_MAX_RAW 2048          /* codes of one explicit text, spaces included */
enum { QV_CORRECT_PREFIX = 1 };          /* call flag */
enum { QV_CORRECT_NO_TARGET = 1, QV_CORRECT_NO_TRANSCRIPT = 2, QV_CORRECT_TOO_LONG = 4, QV_CORRECT_LAST_WORD_OPEN = 8 };   /* row flags */
typedef struct {
    int32_t n_ref, n_pred, n_words, n_ref_used, words_touched, distance;
    int32_t n_match, n_sub, n_del, n_ins, n_ops, flags;
    int32_t start_verse, span;            /* the winner's text (results entry); -1, 0 for explicit texts */
    int32_t reserved[2];
} qv_correct_info;
typedef struct { uint16_t n_symbols, n_match, n_sub, n_del, n_ins, type; } qv_correct_word;

/* explicit texts as alphabet codes WITH their spaces, concatenated: row r compares pred_codes_host[pred_off_host[r] ..
 * pred_off_host[r+1]) with ref_codes_host[ref_off_host[r] .. ref_off_host[r+1]) (offsets as in qv_tracker_match).  Works on
 * an engine without a model; uses the current context's workspace and leaves its batch alone.  Null pointer (the outputs
 * ops_host / words_host excepted), rows < 1, unknown flags, decreasing offsets, a text of more than QV_CORRECT_MAX_RAW codes
 * or a pitch below its cap: QV_ERR_ARG, before anything is launched; rows above max_batch: QV_ERR_CAPACITY. */
int qv_correct(qv_engine *e, const uint8_t *pred_codes_host, const int32_t *pred_off_host,
               const uint8_t *ref_codes_host, const int32_t *ref_off_host, int32_t rows, int32_t flags,
               qv_correct_info *info_host, uint8_t *ops_host, int32_t ops_pitch,
               qv_correct_word *words_host, int32_t words_pitch, void *stream);
/* the rows of context ctx's last batch: pred = the normalised transcript the decode stage left on the device (what
 * qv_debug_transcript_codes returns), ref = the text the winner's token list was tokenised from -- a single verse's clean
 * text; in a span the first ayah without its bismillah where it has one, the rest behind it, single spaces between -- so
 * word k is word k of the word timings.  The winner is chosen as qv_align_results_ctx chooses it (QV_SOURCE_TEXT and
 * QV_SOURCE_CTC alike); a row without a prediction carries QV_CORRECT_NO_TARGET.  Never reads the log-probs.  Lifetime and
 * waiting as qv_nbest_results_ctx: call it before the context is reused, it waits for the batch itself; works after
 * qv_predict_batch[_async[_ctx]] and qv_decode_retrieve_rerank[_async], with either window.  Bad context, null info_host,
 * batch < 1, a batch the context does not hold, unknown flags or a pitch below its cap: QV_ERR_ARG; batch above max_batch:
 * QV_ERR_CAPACITY. */
int qv_correct_results_ctx(qv_engine *e, int32_t ctx, int32_t batch, int32_t flags,
                           qv_correct_info *info_host, uint8_t *ops_host, int32_t ops_pitch,
                           qv_correct_word *words_host, int32_t words_pitch);

/* ---- transcription with confidence --------------------------------------------------------------
 * The greedy transcript of every row together with how sure the model was of it: what a streaming front end gates its
 * chunks by (the reference's transcribers return {"text", "avg_logprob"}, shared/streaming.py:158-181).  One kernel on
 * log-probs f32[batch, t_max, 1025] in HBM with t_host[b] valid frames (rows t >= t_host[b] are never read), one
 * fixed-size record per row back in one copy.
 *   per frame   fid[t] = the argmax of frame t with numpy's first-maximum rule (the decode stage's own rule: -0.0 and
 *               +0.0 tie, the smaller index wins); m[t] = lp[t][fid[t]], float32.
 *   tokens      frame t starts a run if t == 0 or fid[t] != fid[t-1]; blank runs are runs.  Every non-blank run is a token:
 *               id[i], first[i] / last[i] = the run's first and last frame (inclusive; a frame is 0.08 s), logp[i] = the
 *               maximum of m[t] over the run (the value at the first frame that attains it: float32, exact, independent
 *               of the order of evaluation).  The ids are those qv_decode_retrieve_rerank reports as greedy ids.
 *   per row     n_tokens, t_frames, n_blank_frames (frames whose argmax is the blank); min_token_logprob = the smallest
 *               logp[i] (0 without tokens); avg_logprob = sum of logp[i] / n_tokens (0.0 without tokens);
 *               frame_avg_logprob = sum of m[t] / t_frames (0.0 without frames); flags = QV_FLAG_EMPTY_TRANSCRIPT when there
 *               is no token, else 0.
 *   the sums    are float64 and formed in ONE order, so the two averages are reproducible bit for bit: the elements are
 *               converted to double; lane l of 64 adds the elements l, l + 64, l + 128, ... in ascending order starting
 *               from +0.0; the 64 partial sums are combined by p[l] = p[l] + p[l ^ o] for o = 32, 16, 8, 4, 2, 1 (addition
 *               commutes: all lanes end with the same value); one IEEE double division by the count follows.
 *   -inf        maxima propagate as IEEE says (a frame of -inf everywhere yields token 0 with logp = -inf).  Valid frames
 *               hold no NaN.
 * Output rows are `pitch` entries apart, pitch >= t_max.  Entries past n_tokens hold -1 in ids / first / last and 0 in logp.
 * logp_host, first_host and last_host may each be NULL.  NULL info_host / ids_host / input pointer, batch < 1, t_max < 1,
 * pitch < t_max, a t_host[b] outside 0..t_max: QV_ERR_ARG; batch above max_batch or t_max above the engine's frame capacity:
 * QV_ERR_CAPACITY.  The workspace (per row of max_batch a record of 40 + 12 * frame capacity bytes in device memory plus a
 * pinned mirror) belongs to the current execution context and is allocated by the first call that uses it; one
 * device-to-host copy per call.  Independent of the retrieval state: results of an earlier batch stay fetchable. */
typedef struct {
    int32_t n_tokens, t_frames, n_blank_frames, flags;
    float   min_token_logprob, reserved_f;
    double  avg_logprob, frame_avg_logprob;
} qv_transcript_info;

/* on the caller's log-probs; works on an engine without a model.  SYNCHRONOUS on `stream`. */
int qv_transcribe(qv_engine *e, const float *logprobs_dev, const int32_t *t_host, int32_t batch, int32_t t_max,
                  qv_transcript_info *info_host, int32_t *ids_host,
                  float *logp_host, int16_t *first_host, int16_t *last_host,
                  int32_t pitch, void *stream);
/* the forward (as qv_predict_batch runs it: audio_dev f32[batch, n_max], zero padded) into the current context's own log-prob
 * workspace, then the same kernel; t_max = qv_frames_for_samples(longest row).  Waits for batches in flight first (their
 * results stay fetchable, but a batch whose log-probs lived in that workspace is forgotten by qv_align_results_ctx /
 * qv_nbest_results_ctx / qv_debug_transcript_codes: ask them before transcribing).  SYNCHRONOUS like
 * qv_predict_batch.  An engine without a model: QV_ERR_NO_MODEL. */
int qv_transcribe_batch(qv_engine *e, const float *audio_dev, const int64_t *lengths_host,
                        int32_t batch, int64_t n_max,
                        qv_transcript_info *info_host, int32_t *ids_host,
                        float *logp_host, int16_t *first_host, int16_t *last_host,
                        int32_t pitch, void *stream);

/* ---- recordings of any length ---------------------------------------------------------------------
 * qv_create refuses max_samples above 61 s; a longer recording is transcribed through WINDOWS the engine accepts.  All
 * quantities below are encoder frames of 1280 samples: qv_frames_for_samples(n) = n / 1280 + 1, so local frame j of a window
 * that starts at sample 1280 * a is global frame a + j, with no remainder at the recording's end.
 *   Kw   window_samples / 1280.  window_samples: a positive multiple of 1280, at most the engine's max_samples; 0 = the
 *        largest such multiple.
 *   M    margin_frames >= 0: frames not kept at a cut edge; -1 = min(50, Kw / 4) (4 s where it fits).
 *   H    Kw - 2 M >= 1, else QV_ERR_ARG.        T = n / 1280 + 1.
 *   one window if n <= window_samples; otherwise nw = the smallest integer with 1280 * ((nw - 1) * H + Kw) >= n.
 *   window w starts at sample 1280 * w * H, is min(1280 * Kw, n - start) samples long and zero padded behind; the forward
 *        is given that length (a last window of fewer than 400 samples -- M = 0 only -- as 400, the forward's minimum).
 *   window w OWNS the global frames [lo_w, hi_w): lo_0 = 0, else lo_w = w * H + M; hi_(nw-1) = T, else hi_w = (w + 1) * H + M.
 *        The ranges tile [0, T).  Frames a window does not own are never read after the forward.
 * The owned frames' argmax ids and maxima form ONE sequence of T frames, which is collapsed by qv_transcribe's rule, seams
 * included: runs, tokens, logp, n_blank_frames, min_token_logprob and the two float64 averages are defined above, on the
 * global sequence; first / last are global frames (int32).  So the result equals, bit for bit, "qv_forward on every window,
 * keep the owned frames, qv_transcribe's rule on the stitched sequence"; for n <= window_samples it equals qv_transcribe_batch
 * / qv_transcribe field for field.  How close it comes to ONE forward over the whole recording depends on the weights and
 * on M and is not measured.
 * Output rows are `pitch` entries apart, pitch >= the largest T (else QV_ERR_ARG), padded like qv_transcribe's; logp_host,
 * first_host and last_host may each be NULL.  rows above max_batch or T above QV_LONG_MAX_FRAMES: QV_ERR_CAPACITY, before
 * anything is launched or written.  The long workspace (per recording fid, m, one record of 48 + 16 * T bytes, a pinned
 * mirror; with a model the [max_batch, window_samples] batch) is allocated or grown by the first call that needs it and freed
 * by qv_destroy. */
#define QV_LONG_MAX_FRAMES 262144
typedef struct {
    int32_t n_tokens, t_frames, n_blank_frames, flags, n_windows, reserved;
    float   min_token_logprob, reserved_f;
    double  avg_logprob, frame_avg_logprob;
} qv_long_info;

/* the plan alone: host only, no GPU, no engine.  QV_ERR_ARG for bad window / margin values, QV_ERR_CAPACITY above
 * QV_LONG_MAX_FRAMES.  Output pointers may be NULL. */
int qv_long_plan(int64_t n_samples, int32_t max_samples, int32_t window_samples, int32_t margin_frames,
                 int32_t *n_windows, int32_t *t_total, int32_t *kw, int32_t *m);
/* audio_dev: f32[rows, audio_pitch], lengths_host[r] <= audio_pitch samples each (rows <= max_batch).  The windows of all
 * recordings, in recording-then-window order, go through the forward in rounds of max_batch (plain launches into the current
 * context's log-prob workspace).  Waits for batches in flight and forgets the workspace's earlier batch exactly as
 * qv_transcribe_batch does.  SYNCHRONOUS.  An engine without a model: QV_ERR_NO_MODEL; a recording under 400 samples:
 * QV_ERR_CAPACITY like the forward. */
int qv_transcribe_long(qv_engine *e, const float *audio_dev, int64_t audio_pitch, const int64_t *lengths_host, int32_t rows,
                       int32_t window_samples, int32_t margin_frames,
                       qv_long_info *info_host, int32_t *ids_host,
                       float *logp_host, int32_t *first_host, int32_t *last_host,
                       int32_t pitch, void *stream);
/* the same behind the forward: logprobs_dev f32[n_windows_total, t_max, 1025] holds the windows' log-probs in the flattened
 * order, t_max >= Kw + 1 (else QV_ERR_ARG); n_samples_host[rows] the recordings' lengths.  Frames a window does not own and
 * frames past a window's length may hold anything, NaN included.  Works on an engine without a model.  SYNCHRONOUS. */
int qv_transcribe_windows(qv_engine *e, const float *logprobs_dev, int32_t t_max, const int64_t *n_samples_host, int32_t rows,
                          int32_t window_samples, int32_t margin_frames,
                          qv_long_info *info_host, int32_t *ids_host,
                          float *logp_host, int32_t *first_host, int32_t *last_host,
                          int32_t pitch, void *stream);

/* ---- word and verse timings for recordings of any length: long CTC alignment ----------------------
 * The Viterbi contract of "word timings" above -- start state, recursion, tie rule, end rule, float32 with one add per state
 * and frame, `score` reproducible bit for bit, per token first / last / logp -- over the frames of a whole recording and a
 * target of up to QV_ALIGN_LONG_MAX_TOKENS tokens.  lp[t] is the log-prob row of GLOBAL frame t from the window that owns it
 * ("recordings of any length": the same windows, the same rounds, the same ownership); frames a window does not own and
 * frames past a window's length are never read and may hold NaN.  first / last are global frames (int32, inclusive); logp
 * is the float32 sum of lp[t][tgt[i]] over them in ascending t, divided by their count.
 * Flags as qv_align's: QV_ALIGN_NO_TARGET (L == 0), QV_ALIGN_TOO_LONG (L > QV_ALIGN_LONG_MAX_TOKENS), QV_ALIGN_INFEASIBLE
 * (T < L + number of adjacent equal tokens, or a final score below -1e29).  A flagged row holds -1 in first / last and 0 in
 * logp and score, as do the entries past n_tokens; the other rows of the call are unaffected.  For a recording of one window
 * with L <= QV_ALIGN_MAX_TOKENS and T within the engine's capacity the result equals qv_align's on that row, field for field.
 * Row r aligns targets[off[r] ..] (off = running sum of lens_host, ids 0..1023 else QV_ERR_ARG); output rows are `pitch`
 * entries apart, pitch >= the largest lens_host[r] (else QV_ERR_ARG).  Argument checks are those of qv_transcribe_long /
 * qv_transcribe_windows.
 * Workspace (one per engine, grown on need, freed by qv_destroy), in bytes, summed over the rows of a call:
 *     kept rows       T * 1025 * 4, rounded up to a multiple of 16
 *   + back-pointers   T * threads * NS / 4     for a row with 1 <= L <= QV_ALIGN_LONG_MAX_TOKENS, else 0
 * with S = 2 L + 1, NS = 4, 8, 16 or 32 states per thread for S <= 4096, 8192, 16384, 32767, and threads = ceil(S / NS)
 * rounded up to a multiple of 64: two bits per state and frame, padded to the thread layout.  The largest surah (14,403
 * tokens) over 2.5 hours is about 1.3 GB.  Rows above max_batch, T above QV_LONG_MAX_FRAMES or more than
 * QV_ALIGN_LONG_MAX_BYTES (a design limit): QV_ERR_CAPACITY before anything is allocated or launched.  How close windowed
 * log-probs come to one forward over the whole recording is not measured; that limit carries over. */
#define QV_ALIGN_LONG_MAX_TOKENS 16383      /* S <= 32767; the largest surah has 14,403 */
#define QV_ALIGN_LONG_MAX_BYTES 4294967296LL /* 4 GiB */
typedef struct { int32_t n_tokens, flags, t_frames, n_windows; float score, reserved_f; } qv_align_long_info;

/* host only, no GPU, no engine: the windows of all rows and the workspace bytes (the formula above) a call with these rows
 * would need.  QV_ERR_ARG for rows < 1, a null or negative length or token count, bad window / margin values;
 * QV_ERR_CAPACITY above QV_LONG_MAX_FRAMES or QV_ALIGN_LONG_MAX_BYTES (the outputs are written all the same where the
 * frames allow).  Output pointers may be NULL. */
int qv_align_long_plan(const int64_t *n_samples, const int32_t *n_tokens, int32_t rows, int32_t max_samples,
                       int32_t window_samples, int32_t margin_frames, int32_t *n_windows_total, int64_t *bytes);
/* behind the forward, like qv_transcribe_windows (the same logprobs_dev, t_max, n_samples_host): works on an engine without
 * a model.  SYNCHRONOUS. */
int qv_align_windows(qv_engine *e, const float *logprobs_dev, int32_t t_max, const int64_t *n_samples_host, int32_t rows,
                     int32_t window_samples, int32_t margin_frames, const uint16_t *targets_host, const int32_t *lens_host,
                     qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host, float *logp_host,
                     int32_t pitch, void *stream);
/* audio in, as qv_transcribe_long: the same rounds of max_batch windows through the forward, every round's owned rows kept
 * before the next round reuses the log-prob workspace.  Waits for batches in flight and forgets the workspace's earlier batch
 * exactly as qv_transcribe_long does.  SYNCHRONOUS.  QV_ERR_NO_MODEL without a model. */
int qv_align_long(qv_engine *e, const float *audio_dev, int64_t audio_pitch, const int64_t *lengths_host, int32_t rows,
                  int32_t window_samples, int32_t margin_frames, const uint16_t *targets_host, const int32_t *lens_host,
                  qv_align_long_info *info_host, int32_t *first_host, int32_t *last_host, float *logp_host,
                  int32_t pitch, void *stream);

/* ---- verse-constrained beam search ------------------------------------------------------------------
 * A CTC prefix beam search in which every hypothesis is a prefix of a real verse or of a run of up to max_span consecutive
 * verses: it cannot leave the Quran, needs no text matching, and recognises a recitation that stops mid-verse as a prefix
 * with a known set of verses still reachable.  (The reference's second route, web/frontend/src/worker/beam-decode.ts over
 * src/lib/phoneme-trie.ts, with one deliberate difference: DESIGN.md 4.16.)
 *   the trie    for every verse v ascending and every span sp = 1..max_span the token sequence of key v * 6 + sp - 1 of the
 *               tables' token table (what the CTC rerank scores), empty ones skipped; (v, sp) is an END of the sequence's last
 *               node.  Nodes are numbered breadth-first from root = 0, the children of a node in ascending token id.
 *               tok(n) = the token on the edge into node n.  161,465 / 343,929 / 523,170 / 1,046,039 nodes for max_span
 *               1 / 2 / 3 / 6; 8 bytes per node in HBM.  Built and uploaded by the first call that asks for a span, kept until
 *               another span is asked for or qv_destroy.
 *   a state     at most `beam` hypotheses (n, pb, pnb): node, log-probability (float64) of the paths that end in blank / in
 *               non-blank.  Start: {(0, 0.0, -inf)}.  lae(a, b) = b if a == -inf; a if b == -inf; else
 *               max + log1p(exp(min - max)).  tot = lae(pb, pnb).
 *   frame t     row lp[t] (float32, widened exactly).  Every hypothesis stays: pb' = tot + lp[blank], s = pnb + lp[tok(n)]
 *               (s = -inf for the root); and extends into every child c with token k:
 *               x(c) = ((n != 0 && k == tok(n)) ? pb : tot) + lp[k].  A candidate node c gets pb'(c) from its own stay
 *               (else -inf) and pnb'(c) = lae(s(c), x(c)), a missing term taken as -inf.
 *   pruning     candidates whose total is -inf are dropped; the `beam` largest totals are kept, ties to the smaller node.
 *   result      after the last frame the hypotheses by total descending, ties to the smaller node; the first k of them.
 *               max_candidates = the largest number of distinct candidate nodes a frame produced (before the -inf ones are
 *               dropped); no candidate is ever dropped for lack of room.
 * Rows t >= t_host[b] are never read; valid frames hold no NaN.  A row of t_host[b] = 0 returns the start state. */
#define QV_BEAM_MAX 64
enum { QV_BEAM_COMPLETE = 1 };      /* qv_beam_entry.flags: the node is the end of at least one (verse, span) */
typedef struct {
    int32_t node;                   /* trie node of the hypothesis (of the trie for the call's max_span) */
    int32_t n_tokens;               /* its depth */
    int32_t n_ends;                 /* (verse, span) sequences that END here (repeated verses share a node) */
    int32_t start_verse, span;      /* the first of them by (verse, span): global verse index, number of ayat; -1, 0 if none */
    int32_t surah, ayah, ayah_end;  /* ... as a reference; 0, 0, 0 if none */
    int32_t below_count;            /* ends at or under the node: what is still reachable */
    int32_t below_verse, below_span;/* the smallest (verse, span) among them */
    int32_t flags;                  /* QV_BEAM_* */
    double score;                   /* lae(blank_score, nonblank_score) */
    double blank_score, nonblank_score;
} qv_beam_entry;
typedef struct { int32_t n_entries, t_frames, max_candidates, reserved; } qv_beam_info;

/* Statistics of the trie for max_span in 1..6 from a tables file: host only, no engine, no GPU.  Output pointers may be
 * NULL.  QV_ERR_ARG for a bad span, QV_ERR_IO for a file the reader refuses. */
int qv_trie_stats(const char *tables_path, int32_t max_span, int32_t *nodes, int32_t *ends, int32_t *max_depth,
                  int32_t *max_children);
/* The tokens from the root to `node` of the engine's trie for max_span (host-side walk of the parents; builds the trie if
 * the engine does not hold that span).  n_out receives the count; more than `cap` tokens or no such node: QV_ERR_ARG. */
int qv_trie_node_tokens(qv_engine *e, int32_t max_span, int32_t node, int32_t *ids_out, int32_t cap, int32_t *n_out);
/* The search on the caller's log-probs f32[batch, t_max, 1025]; works on an engine without a model.  SYNCHRONOUS on
 * `stream`.  info_host[batch]; entries_host[batch][k], entries past n_entries zeroed; ids_host (may be NULL): row b, `pitch`
 * entries apart (pitch >= t_max), receives the tokens of entry 0, -1 padded.  1 <= beam <= QV_BEAM_MAX, 1 <= k <= beam.
 * One record per row comes back in one copy; the workspace (max_batch records of 2,064 bytes plus a pinned mirror) belongs to
 * the current execution context and is allocated by the first call that uses it.  Null pointers, batch < 1, t_max < 1, beam /
 * k / max_span out of range, pitch < t_max, a t_host[b] outside 0..t_max: QV_ERR_ARG; batch above max_batch or t_max above
 * the engine's frame capacity: QV_ERR_CAPACITY, before anything is launched. */
int qv_beam_decode(qv_engine *e, const float *logprobs_dev, const int32_t *t_host, int32_t batch, int32_t t_max,
                   int32_t max_span, int32_t beam, int32_t k, qv_beam_info *info_host, qv_beam_entry *entries_host,
                   int32_t *ids_host, int32_t pitch, void *stream);
/* the forward (as qv_transcribe_batch runs it, with the same contract: waits for batches in flight, forgets the workspace's
 * earlier batch, QV_ERR_NO_MODEL without a model) into the current context's log-prob workspace, then the same kernel;
 * t_max = qv_frames_for_samples(longest row). */
int qv_beam_batch(qv_engine *e, const float *audio_dev, const int64_t *lengths_host, int32_t batch, int64_t n_max,
                  int32_t max_span, int32_t beam, int32_t k, qv_beam_info *info_host, qv_beam_entry *entries_host,
                  int32_t *ids_host, int32_t pitch, void *stream);

/* ---- exhaustive CTC scan ------------------------------------------------------------------------------
 * Every verse and every run of up to max_span consecutive ayat scored by CTC against the log-probs, the best k returned: the
 * exact, retrieval-free answer to "which verse is this audio" -- no greedy transcript, no text matching, no candidate cap.
 * (The reference's brute-force route, experiments/fastconformer-nbest-bruteforce/run.py over
 * experiments/ctc-alignment/ctc_scorer.py, which a CPU limits to 10 surahs; here the whole table is the default.)
 *   a key       (v, sp): global verse index v in 0 .. n_verses - 1, span sp in 1 .. max_span, 1 <= max_span <= 6.  Its target
 *               is the token sequence of key v * 6 + sp - 1 of the tables' token table (what the CTC rerank scores), L its
 *               length.
 *   feasible    for a row of T frames: L > 0 (the table leaves spans that cross a surah's end, and over-long ones, empty),
 *               2 L + 1 <= T (the reference's gate, ctc_scorer.py:48), and the surah of v selected by the row's surah mask
 *               (bit s - 1 of the 128-bit mask selects surah s; no mask = every surah).  The engine holds at most 766 frames,
 *               so L never exceeds 382.
 *   loss        loss(v, sp) = the float32 negative log-likelihood that qv_debug_ctc_loss returns for that target on the row's
 *               log-probs, bit for bit: the same per-state arithmetic.  One alpha recursion runs per start verse and maximal
 *               run of spans in which each span's ids are a prefix of the next one's, over the longest feasible one; the
 *               shorter ones are read out of its last row (alpha of the states 0 .. 2 P does not depend on what follows the
 *               first P tokens, so sharing changes no bit).
 *   score       norm = loss / L in float32; final = -(double)norm - span_penalty * (sp - 1) in double, each operation rounded
 *               once.  span_penalty = 0.0 gives the order of the reference's brute force (loss / L ascending).
 *   ranking     the feasible keys by final descending, ties to the smaller v, then the smaller sp (repeated verses have
 *               identical targets: exact ties are real).  The first k are returned, 1 <= k <= QV_SCAN_MAX.
 * Rows t >= t_host[b] are never read; valid frames hold finite values.  A row of t_host[b] = 0, or without a feasible key,
 * returns n_entries = 0.  Cost: one state update per frame and state of every recursion -- qv_scan_stats counts them (69 M
 * for T = 126, 595 M for T = 376 on the whole table); timings: DESIGN.md, "exhaustive CTC scan". */
#define QV_SCAN_MAX 32
typedef struct {
    int32_t start_verse, span;      /* the key: global verse index, number of ayat */
    int32_t surah, ayah, ayah_end;  /* ... as a reference; ayah_end = ayah + span - 1 */
    int32_t n_tokens;               /* L */
    float loss, norm;
    double final_score;
} qv_scan_entry;
typedef struct { int32_t n_entries, n_feasible, n_recursions, t_frames; } qv_scan_info;

/* What a row of t_frames frames costs, from a tables file: host only, no engine, no GPU.  surah_mask4: four 32-bit words, NULL =
 * every surah.  n_feasible: feasible keys; n_recursions: alpha recursions that score them; state_steps: the sum over the
 * recursions of (2 L + 1) * t_frames.  Output pointers may be NULL.  QV_ERR_ARG for a null path, t_frames outside 0..768 (two
 * frames above the largest engine's capacity), a bad span or a mask of all zeros; QV_ERR_IO for a file the reader refuses. */
int qv_scan_stats(const char *tables_path, int32_t t_frames, int32_t max_span, const uint32_t *surah_mask4, int32_t *n_feasible,
                  int32_t *n_recursions, int64_t *state_steps);
/* The scan on the caller's log-probs f32[batch, t_max, 1025]; works on an engine without a model.  SYNCHRONOUS on `stream`.
 * surah_mask_host: u32[batch][4] or NULL.  info_host[batch]; entries_host[batch][k], entries past n_entries zeroed.
 * loss_out_dev (may be NULL): the caller's device f32[batch][n_verses * 6]; receives every scored key's loss at v * 6 + sp - 1
 * and +inf everywhere else (empty, infeasible, masked out, sp > max_span).  One record per row comes back in one copy; the
 * workspace (plans, records, 12 bytes per row and key) belongs to the current execution context and is allocated by the first
 * call that uses it.  Null pointers, batch < 1, t_max < 1, max_span / k out of range, a t_host[b] outside 0..t_max, a row mask
 * of all zeros: QV_ERR_ARG; batch above max_batch or t_max above the engine's frame capacity: QV_ERR_CAPACITY, before anything
 * is launched. */
int qv_scan_logprobs(qv_engine *e, const float *logprobs_dev, const int32_t *t_host, int32_t batch, int32_t t_max,
                     int32_t max_span, double span_penalty, int32_t k, const uint32_t *surah_mask_host,
                     qv_scan_info *info_host, qv_scan_entry *entries_host, float *loss_out_dev, void *stream);
/* the forward (as qv_beam_batch runs it, with the same contract: waits for batches in flight, forgets the workspace's
 * earlier batch, QV_ERR_NO_MODEL without a model) into the current context's log-prob workspace, then the same kernels;
 * t_max = qv_frames_for_samples(longest row). */
int qv_scan_batch(qv_engine *e, const float *audio_dev, const int64_t *lengths_host, int32_t batch, int64_t n_max,
                  int32_t max_span, double span_penalty, int32_t k, const uint32_t *surah_mask_host,
                  qv_scan_info *info_host, qv_scan_entry *entries_host, float *loss_out_dev, void *stream);
/* with qv_profile_stages on: milliseconds the last scan spent in the scoring kernel and in the selection kernel */
int qv_scan_kernel_times(qv_engine *e, float *ms2_host);

/* Device pointer of the packed (surah, ayah, ayah_end, float-bits(score)) i32[B,4] rows of the
 * last async call -- the payload of the per-batch RCCL all-gather. */
const int32_t *qv_packed_results_dev(qv_engine *e);

/* ---- stage-level entry points used by the parity tests (each SYNCHRONOUS) ------------- */

/* match_verse/search/pass-3/_build_candidates for one already-normalised transcript given
 * as alphabet codes.  Outputs: base (start verse index, span, score); candidate list in
 * reference order as (start index, span, text score).  cand_cap = capacity of the arrays. */
int qv_debug_retrieve(qv_engine *e, const uint8_t *codes_host, int32_t n_codes,
                      int32_t *base_start, int32_t *base_span, double *base_score,
                      int32_t *cand_start, int32_t *cand_span, double *cand_score,
                      int32_t cand_cap, int32_t *n_cand, int32_t *runner_idx, double *runner_score,
                      int32_t *n_runners, void *stream);

/* CTC negative log-likelihood (float32 alpha recursion) of n target sequences against one
 * [T,1025] log-prob matrix in HBM.  targets_host: concatenated u16 ids, lens_host[n]. */
int qv_debug_ctc_loss(qv_engine *e, const float *logprobs_dev, int32_t t_frames,
                      const uint16_t *targets_host, const int32_t *lens_host, int32_t n,
                      float *loss_host, void *stream);

/* The normalised transcript the decode kernel left in context ctx's workspace -- what the matching kernels read, not a
 * host restatement from the greedy ids.  Row b of codes_host (rows `pitch` bytes apart, pitch >= qv_max_transcript(e),
 * else QV_ERR_ARG) receives the row's len_host[b] alphabet codes (0 = ' ', 63 = a character outside the verse alphabet;
 * bytes past the length are left alone); len_host[b] / words_host[b] = its length in codes and its number of
 * whitespace-separated words.  A row flagged QV_FLAG_EMPTY_TRANSCRIPT or QV_FLAG_TRANSCRIPT_TRUNCATED has length 0.
 * Same lifetime rule as qv_fetch_results_ctx: ask before the context is reused; it waits for the batch itself.  Works
 * with either matching window.  Bad context, null pointer, batch < 1 or a batch the context does not hold: QV_ERR_ARG;
 * batch above max_batch: QV_ERR_CAPACITY. */
int qv_debug_transcript_codes(qv_engine *e, int32_t ctx, int32_t batch, uint8_t *codes_host, int32_t pitch,
                              int32_t *len_host, int32_t *words_host);

/* Intermediate activations of the acoustic model for the layer-wise parity tests.
 * what: 0 = normalised mel features f32[B, t_mel_max, 80]; 1 = subsampling output
 * f32[B, t_max, 512]; 2 = encoder output after layer `layer` f32[B, t_max, 512].
 * QV_PREC_ORT_MIXED only (the tensors in front of / behind each quantiser of the conv path):
 * 3 = norm_conv output, 4 = GLU output, 5 = depthwise conv + BatchNorm + Swish output of layer `layer`,
 * each f32[B, t_max, 512]; 6 = conv.2 output f32[B, t2_max, 20, 256], 7 = ReLU(conv.3) (same shape),
 * 8 = conv.5 output f32[B, t_max, 10, 256], 9 = ReLU(conv.6) f32[B, t_max, 10, 256] (rows past an
 * utterance's length are unspecified for 6..9).  f16 front end only: 11 = conv.2 output (the first depthwise
 * convolution, what k_sub01 or the two-kernel path wrote) converted to f32[B, t2_max, 20, 256], t2_max = the longest
 * clip's count (rows past an utterance's length are that stage's values on zero padding). */
int qv_debug_forward_tap(qv_engine *e, int32_t what, int32_t layer, float *out_dev, void *stream);

/* Measurement hooks for bench.py's roofline line: while enabled, every GEMM launch of the
 * acoustic model is bracketed by HIP events on its own stream.  After synchronising the stream,
 * qv_profile_gemm_read() returns, per kernel class c = epilogue*3 + tile (0 = 64-wide, 1 = 128-wide,
 * 2 = 256 x 256; 21 classes), the summed event time in ms, the summed algorithmic FLOPs (2*M*N*K)
 * and the launch count, and clears the log. */
int qv_profile_gemm(qv_engine *e, int32_t enable);
int qv_profile_gemm_read(qv_engine *e, double *ms21, double *flops21, int32_t *launches21);
/* Replays ONE GEMM of layer 0 with the shapes of the last forward `iters` times back to back
 * between two HIP events on `stream` (SYNCHRONOUS).  which: 0 FFN-up [M,512]x[512,2048]+Swish,
 * 1 FFN-down [M,2048]x[2048,512]+residual, 2 QKV, 3 attention out-projection, 4 pointwise-conv+GLU.
 * Returns the average launch duration in microseconds and the algorithmic FLOPs (2*M*N*K). */
int qv_profile_replay_gemm(qv_engine *e, int32_t which, int32_t iters, double *avg_us, double *flops_per_launch,
                           void *stream);
/* Name of the kernel that replay runs, i.e. the tile shape the launcher picks for that GEMM at the last
 * forward's row count ("k_gemm256<f16_swish>", "k_gemm<resid,128>", ...). */
int qv_profile_replay_kernel(qv_engine *e, int32_t which, char *name_out, int32_t name_cap);
/* Process-wide GEMM tile policy, for the tests that compare tile shapes bit for bit: 0 = 128-wide tiles only,
 * 1 = the default (256 x 256 tiles where N % 256 == 0 and the grid has >= 160 of them), 2 = 256 x 256 wherever
 * the shape allows, -1 = back to the environment (QVERSE_GEMM_T256) / default.  The tile shape never changes
 * a result: both kernels form the same products in the same accumulation order. */
int qv_debug_gemm_tiles(int32_t mode);
/* Tile HEIGHT of the 256-wide kernel: 0 = 256 rows always, 1 = the default (192-row tiles where they save a round of tiles
 * over the 256 CUs and fewer than three batches are in flight), 2 = that rule whatever is in flight, 3 = 192 rows wherever
 * the wide kernel runs, -1 = back to the environment (QVERSE_GEMM_BM) / default.  Same products, same accumulation order:
 * the tile height never changes a result either.  Both switches bump an epoch that is part of the forward-graph key. */
int qv_debug_gemm_tile_height(int32_t mode);
/* Pipeline of the 128- / 64-wide GEMM kernels, the three switches a host sets with QVERSE_GEMM_LD / _NST / _NARROW
 * (INTEGRATION.md 7), for the tests that walk every variant in one process.  ld: 1 = register-staged loader waves (default),
 * 0 = direct global->LDS loads; nst: LDS stages of the direct loads, 2..4 (a 64-wide tile has at most 3), 0 = chosen from
 * the shape; narrow: 1 = 64-wide tiles wherever a kernel of that width exists, 0 = 128-wide wherever N allows.  -1 = that
 * switch back to its variable / default (for narrow: chosen from the shape).  An argument out of range: QV_ERR_ARG, nothing
 * set.  int8 weights and A8W8 only exist 128-wide with register staging and ignore all three.  No variant changes a result.
 * Part of the forward-graph key like the two above; qv_profile_replay_kernel names the pipeline when it is not the
 * default's ("k_gemm<resid,64,lds3>": 64-wide, direct loads, 3 stages). */
int qv_debug_gemm_pipeline(int32_t ld, int32_t nst, int32_t narrow);
/* Process-wide attention kernel variant, for the tests: 3 = the default: an utterance of at most 128 encoder frames
 * (10.2 s) is served by the single-pass short-utterance kernel, a longer one by the key-tiled kernel -- by its OWN length,
 * so the bits of an utterance never depend on the batch it travels in; 0 = the key-tiled kernel (two heads per block)
 * for every utterance, 1 = one head per block, 2 = one wave per query tile, 4 = k_attention_x (key-tiled, four self-staging
 * waves per (head, 128-query group), two blocks per CU) for every utterance, 5 = the short-utterance kernel + k_attention_x;
 * -1 = back to the environment (QVERSE_ATT_X=1 / QVERSE_ATT_TILED=1 / QVERSE_ATT_HPB=1 / QVERSE_ATT_OLD=1, read once per
 * process) / default.  Variants 0, 1, 2, 4 give identical bits, so do 3 and 5; 3 / 5 differ from the others for short
 * utterances by the softmax's summation order only (one pass over the row instead of a running maximum). */
int qv_debug_attention_variant(int32_t mode);

/* Process-wide variant of a single kernel, for the tests that compare two implementations of one stage bit for bit
 * (-1 = back to the environment / default).  which 0 (QVERSE_LOGMEL): the log-mel kernel's 256-point FFT -- 0 = Stockham
 * through LDS, 1 = in registers with DPP / v_permlane*_swap exchanges, 2 = as 1 with a wave walking a run of frames; which 1 (QVERSE_ORT_SUB): conv.0 of
 * QV_PREC_ORT_MIXED's front end -- 0 = VALU, 1 = v_mfma_f32_32x32x2_f32 on the integer-valued operands; which 2
 * (QVERSE_SPANS): match_verse's span pass -- 0 = one LCS walk per span, 1 = one walk per start verse with the count read
 * off at every ayah end; which 3 (QVERSE_FWD_GRAPH): the forward of an engine with more than one context -- 0 = plain
 * launches, 1 = a shape that repeats on a context is captured once and replayed as one hipGraph launch; which 4
 * (QVERSE_CTC): the alpha recursion of the CTC rerank -- 0 = the wave program of rounds 1-5, 1 = the parity-specialised
 * one (two-term log-sum-exp for blank states); which 5 (QVERSE_SUB_RUN): how many tiles of four conv.2 frames one block
 * of the fused subsampling kernel walks -- 0 = chosen from the launch shape, 1 / 2 = one / two tiles, 3 = the most a block
 * ever walks (16), 4 = the most it walks with the run's mel rows resident in LDS (4).  The variants of a kernel produce identical bits. */
int qv_debug_kernel_variant(int32_t which, int32_t mode);

/* The forward's own frame arithmetic, for the tests: frames_out[0..3] = log-mel frames of a clip of n_samples and its
 * frame counts after conv.0, conv.2 and conv.5 (the last one is the encoder's); run_tiles_out (optional) = tiles of four
 * conv.2 frames a block of the fused subsampling kernel walks when `batch` clips, the longest of n_samples, are launched
 * under the current which-5 variant. */
int qv_debug_sub01_plan(int64_t n_samples, int32_t batch, int32_t *frames_out, int32_t *run_tiles_out);
/* ... and of the kernel behind it (conv.3 + conv.5 fused, which 6, no environment variable: 0 = chosen from the launch shape, 1 / 2 =
 * one / two steps of three conv.5 frames, 3 = the most a block ever walks, 16 steps): run_frames_out = conv.5 frames one block
 * walks when `batch` clips, the longest of n_samples, are launched under the current which-6 variant. */
int qv_debug_sub35_plan(int64_t n_samples, int32_t batch, int32_t *run_frames_out);

/* How many forwards of this engine were replayed as a hipGraph launch, and how many graphs were captured, since creation
 * (tests / bench.py: shows that the replay path -- and not the plain launches -- is what ran). */
int qv_debug_forward_graph_stats(qv_engine *eng, int64_t *replays, int64_t *captures);
/* Captures / graph instantiations that failed since creation (a capture-unsafe call of the host invalidated one, ...): the
 * batch is then issued as plain launches and the context stops capturing -- never an error of the batch.  -1: no model. */
int64_t qv_debug_forward_graph_failures(qv_engine *eng);

/* Measurement hook for bench.py's `realistic_mix` leg.  Seeded random weights decode every synthetic clip to a near-empty
 * transcript, so the headline workload never sees a recitation the text match recognises.  While log-probs are injected,
 * qv_predict_batch_async() still runs the WHOLE forward pass on the audio it is given, but its post-logits stages read the
 * caller's tensor (f32[batch, t_max, 1025] in HBM, t_host[b] valid frames; must stay alive and unchanged) instead of the
 * forward's output -- e.g. verse-shaped log-probs at the v1 corpus' gate pass / fail ratio.  NULL clears the hook.  Results
 * are then predictions for the INJECTED log-probs; never use it outside measurements. */
int qv_profile_inject_logprobs(qv_engine *e, const float *logprobs_dev, int32_t t_max, const int32_t *t_host, int32_t batch);

/* Stage timers -- the device-side counterpart of C2C_DIRECT_MIXED_PROFILE (experiments/c2c-direct-mixed/
 * run.py:34,76-81,117-124: forward= decode= build= rerank= per file).  While enabled, every batch brackets
 * its four stages with HIP events on the stream it runs on: forward (acoustic model), decode (argmax +
 * greedy collapse + normalisation), build (match_verse / search / pass 3 / candidate assembly), rerank
 * (CTC losses + decision).  qv_stage_times() waits for context `ctx`'s last batch (SYNCHRONOUS) and
 * returns the four durations in milliseconds; a stage that did not run reports 0. */
int qv_profile_stages(qv_engine *e, int32_t enable);
int qv_stage_times(qv_engine *e, int32_t ctx, float *ms4_host);
/* ... and while enabled, qv_transcribe_long / qv_transcribe_windows bracket every launch of their own three kernels: the last
 * call's milliseconds in k_long_gather, k_long_frames and k_long_collapse (summed over the rounds).  QV_ERR_ARG without one. */
int qv_long_kernel_times(qv_engine *e, float *ms3_host);
/* ... and qv_align_long / qv_align_windows theirs: the last call's milliseconds in k_long_keep (summed over the rounds) and in
 * k_align_long (one launch per instantiation in use; the recordings of a launch run side by side). */
int qv_align_long_kernel_times(qv_engine *e, float *ms2_host);

/* Host-only: block-128 symmetric int4 quantisation of one Linear weight w[N][K] (f32 row-major,
 * N % 64 == 0, K % 128 == 0) followed by the inverse of the device packing, i.e. the f32 matrix
 * (q - 8) * half(scale) the W4A16 GEMM multiplies by under QV_PREC_MIXED_INT4_INT8.  Needs no GPU;
 * the parity tests compare it with the oracle's quantiser. */
int qv_debug_int4_roundtrip(const float *w, int32_t n_rows, int32_t k, float *out);
/* Same for the pointwise-convolution weights of that precision mode: per-output-channel symmetric int8
 * (N % 64 == 0, K % 64 == 0), i.e. the f32 matrix q * scale[n] the W8A16 GEMM multiplies by. */
int qv_debug_int8_roundtrip(const float *w, int32_t n_rows, int32_t k, float *out);

/* Host-only (no GPU needed): the float32 tensors a weight file must hold, in file order -- names are
 * the NeMo state-dict keys of the CTC branch -- and tensor `index` of the seeded synthetic
 * initialisation an engine created with weights_path == NULL uses.  tools/convert_weights.py is
 * written against these, so the converter and the engine cannot disagree about names or shapes. */
int32_t qv_weight_count(void);
int qv_weight_spec(int32_t index, char *name_out, int32_t name_cap, int32_t *dims4_out, int32_t *ndim_out);
int qv_weight_random(uint64_t seed, int32_t index, float *out, int64_t numel);

/* What the engine's acoustic model actually runs on, as text: the precision mode and where the quantisation grids came
 * from -- "weights quantised by the engine", or for a file converted from the reference's quantised ONNX
 * (tools/convert_weights.py --onnx marks it) how many Linear tensors sit on the FILE's own MatMulNBits grid and how many
 * run as dequantised f16 values (block sizes other than 128).  bench.py / the plugin report it next to a number. */
int qv_weights_info(qv_engine *e, char *out, int32_t cap);

/* Library build info: "gfx950;hip-x.y;..." */
const char *qv_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* QVERSE_H */
