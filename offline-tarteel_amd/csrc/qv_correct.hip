// qv_correct.hip -- recitation correction: which words of the verse did the reciter get wrong?  (include/qverse.h:
// qv_correct, qv_correct_results_ctx; the rule restated there is shared/phoneme_aligner.py's Levenshtein alignment with its
// tie order S, D, I, folded into words as web/frontend/src/lib/correction.ts folds it.)
//
// k_correct: one workgroup of 128 threads per row, three phases.
//   strip     both texts lose their spaces in the kernel (one definition of "spaceless" for the explicit entry and for the
//             transcript k_decode left in QvWork::q): a block-wide ordered compaction; word(r) = raw index of symbol r - r.
//   sweep     anti-diagonals d = i + j of the DP.  Thread t owns the 16 rows i = 16t .. 16t+15 for the whole sweep, so the
//             two previous diagonals of its rows live in its REGISTERS (cell (i, j) needs (i-1, j) and (i, j-1) of d-1 and
//             (i-1, j-1) of d-2); only the value of row 16t+15 crosses to thread t+1, through a two-deep LDS exchange, one
//             barrier per diagonal.  The reference symbols of the 16 rows are registers too, the predicted symbols a 16-deep
//             register window that shifts by one per diagonal.  Cells outside the matrix hold CR_BIG, so the borders fall out
//             of the recurrence and only dp[0][0] is planted.  The thread's 16 moves of a diagonal are one uint32 (2 bits
//             per cell: 0 S, 1 D, 2 I) stored whole to HBM, diagonal-major: no atomics, no shared words.  In prefix mode the
//             owner of row i sees dp[i][m] pass on diagonal i + m and keeps its smallest (value, i); one LDS min follows.
//   backtrace a dependent chain of at most n + m steps, walked by thread 0 over back-pointers the whole block fetched ahead:
//             a step moves to row i-1 of d-2 (S), row i-1 of d-1 (D) or row i of d-1 (I), so 64 diagonals below the current
//             one can only touch rows i-63 .. i, five words per diagonal -- one block of 64 x 5 words per HBM latency
//             instead of one latency per step (the BCH-rows-ahead scheme of align_wave's backward pass).  The walk leaves
//             (position << 2 | op) per column in LDS, last column first; one parallel pass writes the op codes and adds the
//             per-word counters with LDS atomics (match | sub and del | ins packed in two words, the first error by
//             atomicMin on column << 2 | op), then the words and the info are written.
// LDS (all dynamic): 14,784 bytes with the default window, 17,856 with the wide one (cr_lds below).  Back-pointers:
// (QV_CORRECT_MAX_REF + window + 1) diagonals x 81 words = 746,820 bytes per row (default window), 1,078,596 (wide), for at
// most QV_CORRECT_ROUND = 64 rows: 47.8 MB / 69.0 MB per context that asks, nothing for one that never does.
#include "qv_common.h"
#include "qv_rows.h"

namespace {

constexpr int CR_THREADS = 128;
constexpr int CR_CELLS = 16;                                             // rows of the DP one thread owns
constexpr int CR_BPW = (QV_CORRECT_MAX_REF + CR_CELLS) / CR_CELLS;       // 81 words hold rows 0 .. QV_CORRECT_MAX_REF of a diagonal
constexpr int CR_RAW_PER = QV_CORRECT_MAX_RAW / CR_THREADS;              // raw codes a thread strips
constexpr int CR_BLK_D = 64, CR_BLK_W = CR_BLK_D / CR_CELLS + 1;         // the back-trace's fetch block: diagonals x words
constexpr uint32_t CR_NO_ERR = 0xFFFFFFFFu;
constexpr int CR_BIG = 0x4000;                                           // a cell outside the matrix: above every distance, fits the uint16 exchange with room to grow
static_assert(CR_BPW <= CR_THREADS && CR_RAW_PER * CR_THREADS == QV_CORRECT_MAX_RAW, "one thread per back-pointer word / raw chunk");
static_assert(QV_CORRECT_MAX_REF < (1 << 14), "position << 2 | op in 16 bits");
static_assert(sizeof(qv_correct_info) == 64 && sizeof(qv_correct_word) == 12, "record layout");

// what the kernel reads of the batch and of the tables (results entry; pointers, not QvWork / QvTables by value: the kernel
// has no scalar registers to spare for kernel arguments it never uses)
struct CrBatch {
    const qv_result *results;
    const QvUtt *utt;
    const uint8_t *q;
    const int32_t *cand_start, *cand_span;
    const uint8_t *clean;
    const uint32_t *clean_off;
    const uint16_t *clean_len, *nobsm_len;
    int n_verses;
};

struct CrArgs {
    const uint8_t *codes;      // explicit texts: every pred text, then every ref text; nullptr = the rows of the batch in `bt`
    const int32_t *off;        // [rows + 1] pred offsets, [rows + 1] ref offsets into codes
    int rows_total, row0;      // rows of the call, first row of this round
    int max_q, flags, ops_cap;
    uint32_t *bp;              // [round][ops_cap + 1][CR_BPW]
    size_t bp_row_words;
    unsigned char *out;        // [rows][row_bytes]
    size_t row_bytes;
    CrBatch bt;
};

// LDS carve, every offset a multiple of 16
struct CrLds { int edge, pred, ref, word, rev, cnt, blk, misc, total; };
__host__ __device__ inline CrLds cr_lds(int max_q) {
    auto up = [](int n) { return (n + 15) & ~15; };
    CrLds l;
    int o = 0;
    l.edge = o; o += up(2 * CR_THREADS * 2);                         // uint16 [2][threads]: row 16t+15 of the last two diagonals
    l.pred = o; o += up(max_q);                                      // uint8 stripped pred
    l.ref = o;  o += up(QV_CORRECT_MAX_REF);                         // uint8 stripped ref
    l.word = o; o += up(QV_CORRECT_MAX_REF * 2);                     // uint16 word(r)
    l.rev = o;  o += up((QV_CORRECT_MAX_REF + max_q) * 2);           // uint16 columns, last first
    l.cnt = o;  o += up(QV_CORRECT_MAX_WORDS * 3 * 4);               // uint32 [words][3]
    l.blk = o;  o += up(CR_BLK_D * CR_BLK_W * 4);                    // uint32 fetched back-pointers
    l.misc = o; o += 64;                                             // int32 [16]: scans, state, totals
    l.total = o;
    return l;
}

// Ordered compaction of the non-space codes of src[0 .. raw) into dst (at most cap of them are stored; all are counted);
// wd[r] = spaces in front of symbol r.  scan: two ints of LDS nobody else touches during the call.  Returns the count.
__device__ int cr_strip(const uint8_t *__restrict__ src, int raw, uint8_t *dst, int cap, uint16_t *wd, int *scan) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, base = tid * CR_RAW_PER;
    uint8_t c[CR_RAW_PER];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < CR_RAW_PER; ++k) {
        c[k] = base + k < raw ? src[base + k] : 0;
        cnt += c[k] != 0;
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) scan[wave] = inc;
    __syncthreads();
    int pos = inc - cnt + (wave ? scan[0] : 0);
#pragma unroll
    for (int k = 0; k < CR_RAW_PER; ++k)
        if (c[k] != 0) {
            if (pos < cap) {
                dst[pos] = c[k];
                if (wd) wd[pos] = (uint16_t)(base + k - pos);
            }
            ++pos;
        }
    return scan[0] + scan[1];
}

__global__ __launch_bounds__(CR_THREADS) void k_correct(CrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CrLds L = cr_lds(a.max_q);
    uint16_t *s_edge = (uint16_t *)(smem + L.edge);
    uint8_t *s_pred = smem + L.pred, *s_ref = smem + L.ref;
    uint16_t *s_word = (uint16_t *)(smem + L.word), *s_rev = (uint16_t *)(smem + L.rev);
    uint32_t *s_cnt = (uint32_t *)(smem + L.cnt), *s_blk = (uint32_t *)(smem + L.blk);
    int *s_misc = (int *)(smem + L.misc);   // 0..3 scans, 4 i, 5 j, 6 columns so far, 7 prefix key, 8..11 totals, 12 words touched

    const int tid = threadIdx.x, slot = blockIdx.x, b = a.row0 + slot;
    unsigned char *rec = a.out + (size_t)b * a.row_bytes;
    uint8_t *o_ops = rec + sizeof(qv_correct_info);
    qv_correct_word *o_words = (qv_correct_word *)(o_ops + a.ops_cap);

    // ---- the two texts
    const uint8_t *p_src = nullptr, *r_src = nullptr;
    int p_raw = 0, r_raw = 0, start = -1, span = 0, flags = 0;
    if (a.codes) {
        const int32_t *po = a.off, *ro = a.off + a.rows_total + 1;
        p_src = a.codes + po[b]; p_raw = po[b + 1] - po[b];
        r_src = a.codes + ro[b]; r_raw = ro[b + 1] - ro[b];
    } else {
        const CrBatch &wk = a.bt, &tab = a.bt;
        const qv_result &res = wk.results[b];
        const QvUtt &u = wk.utt[b];
        p_src = wk.q + (size_t)b * a.max_q;
        p_raw = u.q_len < 0 ? 0 : (u.q_len > a.max_q ? a.max_q : u.q_len);
        int st = -1, sp = 0;   // the winner, as k_align_plan selects it
        if (res.surah != 0 && !(res.flags & QV_FLAG_TRANSCRIPT_TRUNCATED)) {
            if (res.source == QV_SOURCE_CTC && u.win >= 0 && u.win < QV_CAND_CAP) {
                st = wk.cand_start[(size_t)b * QV_CAND_CAP + u.win];
                sp = wk.cand_span[(size_t)b * QV_CAND_CAP + u.win];
            } else if (res.source == QV_SOURCE_TEXT) {
                st = u.base_start;
                sp = u.base_span;
            }
        }
        if (st >= 0 && sp >= 1 && sp <= QV_MAX_SPAN && st + sp <= tab.n_verses) {
            // one slice of `clean`: a single verse whole; in a span the first ayah from behind its bismillah
            const uint32_t lo = tab.clean_off[st] + (sp > 1 && tab.nobsm_len[st] ? tab.clean_len[st] - tab.nobsm_len[st] : 0);
            const uint32_t hi = tab.clean_off[st + sp - 1] + tab.clean_len[st + sp - 1];
            r_src = tab.clean + lo;
            r_raw = (int)(hi - lo);
            start = st;
            span = sp;
        }
    }
    if (p_raw > QV_CORRECT_MAX_RAW) { p_raw = QV_CORRECT_MAX_RAW; flags |= QV_CORRECT_TOO_LONG; }
    if (r_raw > QV_CORRECT_MAX_RAW) { r_raw = QV_CORRECT_MAX_RAW; flags |= QV_CORRECT_TOO_LONG; }

    for (int w = tid; w < QV_CORRECT_MAX_WORDS * 3; w += CR_THREADS) s_cnt[w] = w % 3 == 2 ? CR_NO_ERR : 0u;
    if (tid < 16) s_misc[tid] = tid == 7 ? 0x7FFFFFFF : 0;
    __syncthreads();
    const int m = cr_strip(p_src, p_raw, s_pred, a.max_q, nullptr, s_misc + 0);
    const int n = cr_strip(r_src, r_raw, s_ref, QV_CORRECT_MAX_REF, s_word, s_misc + 2);
    const int n_words = 1 + r_raw - n;
    if (n == 0) flags |= QV_CORRECT_NO_TARGET;
    if (m == 0) flags |= QV_CORRECT_NO_TRANSCRIPT;
    if (n > QV_CORRECT_MAX_REF || m > a.max_q || n_words > QV_CORRECT_MAX_WORDS) flags |= QV_CORRECT_TOO_LONG;
    if (flags) {   // (the same in every thread) no ops, no words, every other field 0
        for (int f = tid; f < a.ops_cap; f += CR_THREADS) o_ops[f] = 0xFF;
        for (int w = tid; w < QV_CORRECT_MAX_WORDS; w += CR_THREADS) o_words[w] = qv_correct_word{0, 0, 0, 0, 0, 0};
        if (tid == 0) {
            qv_correct_info inf = {};
            inf.flags = flags;
            *(qv_correct_info *)rec = inf;
        }
        return;
    }
    __syncthreads();   // the stripped texts are in LDS

    // ---- sweep
    uint32_t *bp = a.bp + (size_t)slot * a.bp_row_words;
    const int i0 = tid * CR_CELLS;
    const bool prefix = a.flags & QV_CORRECT_PREFIX;
    int best_v = 0x7FFFF, best_i = 0;
    const bool active = i0 <= n;   // (false in the whole second wave when n < 1024: it only keeps the barriers)
    // Cells outside the matrix hold CR_BIG (and grow by at most one per diagonal), so the borders need no case of their own:
    // dp[i][0] = dp[i-1][0] + 1 is the deletion, dp[0][j] = dp[0][j-1] + 1 the insertion; only dp[0][0] = 0 is planted.
    int p1[CR_CELLS], p2[CR_CELLS], rc[CR_CELLS], pw[CR_CELLS];
#pragma unroll
    for (int k = 0; k < CR_CELLS; ++k) {
        const int i = i0 + k;
        p1[k] = p2[k] = CR_BIG;
        rc[k] = i >= 1 && i <= n ? s_ref[i - 1] : 0x100;
        pw[k] = 0x200;
    }
    int left2 = CR_BIG;
    s_edge[tid] = s_edge[CR_THREADS + tid] = CR_BIG;
    __syncthreads();
    for (int d = 0; d <= n + m; ++d) {   // one barrier per diagonal, met by every thread (no barrier under a divergent branch)
        if (active) {
            const int left1 = tid > 0 ? s_edge[((d + 1) & 1) * CR_THREADS + tid - 1] : CR_BIG;   // row i0-1 of diagonal d-1
#pragma unroll
            for (int k = CR_CELLS - 1; k > 0; --k) pw[k] = pw[k - 1];
            const int jn = d - i0 - 1;                                                             // pred index of cell 0
            pw[0] = jn >= 0 && jn < m ? s_pred[jn] : 0x200;
            uint32_t bits = 0;
#pragma unroll
            for (int k = CR_CELLS - 1; k >= 0; --k) {   // downwards: cell k reads rows k-1 before they are replaced
                const int up1 = k ? p1[k ? k - 1 : 0] : left1, up2 = k ? p2[k ? k - 1 : 0] : left2;
                const int sub = up2 + (rc[k] != pw[k]), del = up1 + 1, ins = p1[k] + 1;
                const int v = min(sub, min(del, ins));
                bits |= (v == sub ? 0u : (v == del ? 1u : 2u)) << (2 * k);
                p2[k] = p1[k];
                p1[k] = v;
            }
            if (d == 0 && tid == 0) p1[0] = 0;
            left2 = left1;
            s_edge[(d & 1) * CR_THREADS + tid] = (uint16_t)p1[CR_CELLS - 1];
            // the cells of this diagonal inside the matrix proper (1 <= i <= n, 1 <= j <= m) among the thread's 16
            const int lo = max(max(i0, 1), d - m) - i0, hi = min(min(i0 + CR_CELLS - 1, n), d - 1) - i0;
            if (lo <= hi) bp[(size_t)d * CR_BPW + tid] = bits & (uint32_t)(((1ull << (2 * hi + 2)) - 1ull) & ~((1ull << (2 * lo)) - 1ull));
            const int kk = d - m - i0;           // the cell of the last column, dp[i][m], if this thread owns it
            if (prefix && kk >= 0 && kk < CR_CELLS && i0 + kk <= n) {
                int v = 0;
#pragma unroll
                for (int k = 0; k < CR_CELLS; ++k) v = k == kk ? p1[k] : v;
                if (v < best_v) { best_v = v; best_i = i0 + kk; }
            }
        }
        __syncthreads();
    }
    if (prefix && best_v < 0x7FFFF) atomicMin(&s_misc[7], best_v * 2048 + best_i);
    __threadfence_block();
    __syncthreads();   // every back-pointer of the row is written (the block's own stores: visible to it after the barrier)
    const int i_end = prefix ? (s_misc[7] & 2047) : n;
    if (tid == 0) { s_misc[4] = i_end; s_misc[5] = m; s_misc[6] = 0; }
    __syncthreads();

    // ---- backtrace
    for (;;) {
        const int i = s_misc[4], j = s_misc[5];
        if (i == 0 || j == 0) break;
        const int d = i + j, d_lo = max(d - (CR_BLK_D - 1), 2), w0 = max(i - (CR_BLK_D - 1), 0) >> 4, w1 = i >> 4;
        for (int x = tid; x < CR_BLK_D * CR_BLK_W; x += CR_THREADS) {
            const int dd = d_lo + x / CR_BLK_W, w = w0 + x % CR_BLK_W;
            if (dd <= d && w <= w1) s_blk[x] = bp[(size_t)dd * CR_BPW + w];
        }
        __syncthreads();
        if (tid == 0) {
            int ci = i, cj = j, k = s_misc[6];
            while (ci > 0 && cj > 0 && ci + cj >= d_lo) {
                const uint32_t wv = s_blk[(ci + cj - d_lo) * CR_BLK_W + ((ci >> 4) - w0)];
                const uint32_t mv = (wv >> ((ci & 15) * 2)) & 3u;
                if (mv == 0) {
                    s_rev[k++] = (uint16_t)(((ci - 1) << 2) | (s_ref[ci - 1] == s_pred[cj - 1] ? 0 : 1));
                    --ci; --cj;
                } else if (mv == 1) {
                    s_rev[k++] = (uint16_t)(((ci - 1) << 2) | 2);
                    --ci;
                } else {
                    s_rev[k++] = (uint16_t)((ci << 2) | 3);
                    --cj;
                }
            }
            s_misc[4] = ci; s_misc[5] = cj; s_misc[6] = k;
        }
        __syncthreads();
    }
    // the border: at i == 0 insertions in front of the first symbol, at j == 0 deletions
    const int ri = s_misc[4], rj = s_misc[5], k0 = s_misc[6], n_ops = k0 + ri + rj;
    for (int x = tid; x < ri + rj; x += CR_THREADS) s_rev[k0 + x] = ri ? (uint16_t)(((ri - 1 - x) << 2) | 2) : (uint16_t)3;
    __syncthreads();

    // ---- ops, words, info
    int c_op[4] = {0, 0, 0, 0};
    for (int f = tid; f < a.ops_cap; f += CR_THREADS) {
        if (f >= n_ops) { o_ops[f] = 0xFF; continue; }
        const int v = s_rev[n_ops - 1 - f], op = v & 3, pos = v >> 2;
        o_ops[f] = (uint8_t)op;
        const int w = s_word[pos < n ? pos : n - 1];
        atomicAdd(&s_cnt[w * 3 + (op >> 1)], (op & 1) ? 0x10000u : 1u);
        if (op) atomicMin(&s_cnt[w * 3 + 2], ((uint32_t)f << 2) | (uint32_t)op);
        c_op[0] += op == 0; c_op[1] += op == 1; c_op[2] += op == 2; c_op[3] += op == 3;
    }
    int touched = 0;
    for (int r = tid; r < i_end; r += CR_THREADS) touched += r == 0 || s_word[r] != s_word[r - 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) c_op[q] += __shfl_xor(c_op[q], o);
        touched += __shfl_xor(touched, o);
    }
    if ((tid & 63) == 0) {
        for (int q = 0; q < 4; ++q) atomicAdd(&s_misc[8 + q], c_op[q]);
        atomicAdd(&s_misc[12], touched);
    }
    __syncthreads();
    for (int w = tid; w < QV_CORRECT_MAX_WORDS; w += CR_THREADS) {
        qv_correct_word o = {0, 0, 0, 0, 0, 0};
        if (w < n_words) {
            const uint32_t ms = s_cnt[w * 3], di = s_cnt[w * 3 + 1], fe = s_cnt[w * 3 + 2];
            o.n_match = ms & 0xFFFF; o.n_sub = ms >> 16; o.n_del = di & 0xFFFF; o.n_ins = di >> 16;
            o.n_symbols = o.n_match + o.n_sub + o.n_del;
            o.type = o.n_sub ? 1 : (fe == CR_NO_ERR ? 0 : (uint16_t)(fe & 3u));
        }
        o_words[w] = o;
    }
    if (tid == 0) {
        qv_correct_info inf = {};
        inf.n_ref = n; inf.n_pred = m; inf.n_words = n_words; inf.n_ref_used = i_end; inf.words_touched = s_misc[12];
        inf.n_match = s_misc[8]; inf.n_sub = s_misc[9]; inf.n_del = s_misc[10]; inf.n_ins = s_misc[11];
        inf.distance = inf.n_sub + inf.n_del + inf.n_ins;
        inf.n_ops = n_ops;
        inf.flags = i_end >= 1 && i_end < n && s_word[i_end - 1] == s_word[i_end] ? QV_CORRECT_LAST_WORD_OPEN : 0;
        inf.start_verse = start; inf.span = span;
        *(qv_correct_info *)rec = inf;
    }
}

}  // namespace

// The correction workspace of one context (QvCorrectWs, qv_common.h), allocated by the first call that uses it.
static int correct_ws(qv_engine *eng, QvCtx &c, QvCorrectWs **out) {
    QvCorrectWs &w = c.correct;
    *out = &w;
    if (w.m.dev) return QV_OK;
    const auto up256 = [](size_t n) { return (n + 255) & ~(size_t)255; };   // every part as aligned as an allocation of its own
    const size_t B = (size_t)c.work.max_batch, ops_cap = (size_t)QV_CORRECT_MAX_REF + eng->max_q;
    const size_t row_bytes = qv_up16(sizeof(qv_correct_info) + ops_cap + QV_CORRECT_MAX_WORDS * sizeof(qv_correct_word));
    const size_t n_out = up256(B * row_bytes), n_in = up256(qv_up16(2 * (B + 1) * sizeof(int32_t)) + B * 2 * QV_CORRECT_MAX_RAW);
    const size_t bp_row_words = (ops_cap + 1) * CR_BPW, slots = B < QV_CORRECT_ROUND ? B : QV_CORRECT_ROUND;
    QvMirror m;
    QV_TRY_RC(qv_ctx_mirror(eng, c, n_out + n_in + slots * bp_row_words * sizeof(uint32_t), n_out + n_in, "correction workspace", &m));
    w.m = m;
    w.row_bytes = row_bytes; w.ops_cap = ops_cap; w.in_off = n_out; w.bp_off = n_out + n_in; w.bp_row_words = bp_row_words;
    return QV_OK;
}

// rounds of QV_CORRECT_ROUND rows on `stream` (one after the other: they share the back-pointers), one copy back, the scatter
static int correct_run(qv_engine *eng, QvCtx &c, QvCorrectWs &w, CrArgs a, int rows, qv_correct_info *info_host, uint8_t *ops_host,
                       int ops_pitch, qv_correct_word *words_host, int words_pitch, hipStream_t stream) {
    a.rows_total = rows;
    a.max_q = eng->max_q;
    a.ops_cap = (int)w.ops_cap;
    a.bp = (uint32_t *)(w.m.dev + w.bp_off);
    a.bp_row_words = w.bp_row_words;
    a.out = w.m.dev;
    a.row_bytes = w.row_bytes;
    const QvTables &t = eng->tab;
    a.bt = {c.work.results, c.work.utt, c.work.q, c.work.cand_start, c.work.cand_span, t.clean, t.clean_off, t.clean_len, t.nobsm_len,
            t.n_verses};
    const size_t lds = (size_t)cr_lds(eng->max_q).total;
    for (int r0 = 0; r0 < rows; r0 += QV_CORRECT_ROUND) {
        a.row0 = r0;
        const int nr = rows - r0 < QV_CORRECT_ROUND ? rows - r0 : QV_CORRECT_ROUND;
        hipLaunchKernelGGL(k_correct, dim3(nr), dim3(CR_THREADS), lds, stream, a);
        QV_HIP(hipGetLastError());
    }
    QV_TRY_RC(qv_fetch_sync(eng, w.m.host, w.m.dev, (size_t)rows * w.row_bytes, stream));
    const qv_correct_word none = {0, 0, 0, 0, 0, 0};
    for (int r = 0; r < rows; ++r) {
        const unsigned char *rec = w.m.host + (size_t)r * w.row_bytes;
        memcpy(&info_host[r], rec, sizeof(qv_correct_info));
        scatter_column<uint8_t>(ops_host, ops_pitch, r, rec + sizeof(qv_correct_info), (int)w.ops_cap, 0xFF);
        scatter_column<qv_correct_word>(words_host, words_pitch, r, (const qv_correct_word *)(rec + sizeof(qv_correct_info) + w.ops_cap),
                                        QV_CORRECT_MAX_WORDS, none);
    }
    return QV_OK;
}

int qv_correct_rows(qv_engine *eng, QvCtx &c, const uint8_t *pred_codes, const int32_t *pred_off, const uint8_t *ref_codes,
                    const int32_t *ref_off, int rows, int flags, qv_correct_info *info_host, uint8_t *ops_host, int ops_pitch,
                    qv_correct_word *words_host, int words_pitch, hipStream_t stream) {
    QvCorrectWs *w = nullptr;
    QV_TRY_RC(correct_ws(eng, c, &w));
    // offsets rebased to the staged buffer (every pred text, then every ref text) and the codes, up in ONE copy
    unsigned char *in_host = w->m.host + w->in_off;
    int32_t *off = (int32_t *)in_host;
    const size_t off_bytes = qv_up16(2 * ((size_t)rows + 1) * sizeof(int32_t));
    uint8_t *codes = in_host + off_bytes;
    int32_t at = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const uint8_t *src = pass ? ref_codes : pred_codes;
        const int32_t *so = pass ? ref_off : pred_off;
        int32_t *o = off + pass * (rows + 1);
        for (int r = 0; r < rows; ++r) {
            const int32_t len = so[r + 1] - so[r];
            o[r] = at;
            if (len) memcpy(codes + at, src + so[r], (size_t)len);
            at += len;
        }
        o[rows] = at;
    }
    const size_t in_bytes = off_bytes + (size_t)at;
    QV_HIP(hipMemcpyAsync(w->m.dev + w->in_off, in_host, in_bytes, hipMemcpyHostToDevice, stream));
    CrArgs a = {};
    a.off = (const int32_t *)(w->m.dev + w->in_off);
    a.codes = w->m.dev + w->in_off + off_bytes;
    a.flags = flags;
    return correct_run(eng, c, *w, a, rows, info_host, ops_host, ops_pitch, words_host, words_pitch, stream);
}

int qv_correct_results(qv_engine *eng, int k_ctx, int batch, int flags, qv_correct_info *info_host, uint8_t *ops_host, int ops_pitch,
                       qv_correct_word *words_host, int words_pitch) {
    QvCtx &c = eng->ctx[k_ctx];
    if (!c.al_lp || batch > c.al_batch) {
        qv_set_error(eng, "qv_correct_results_ctx: the context holds no batch of that size (ask before the context is reused)");
        return QV_ERR_ARG;
    }
    QvCorrectWs *w = nullptr;
    QV_TRY_RC(correct_ws(eng, c, &w));
    hipStream_t stream = nullptr;
    QV_TRY_RC(qv_stream_behind_batch(eng, c, &stream));
    CrArgs a = {};
    a.flags = flags;
    return correct_run(eng, c, *w, a, batch, info_host, ops_host, ops_pitch, words_host, words_pitch, stream);
}
