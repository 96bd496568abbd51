// qv_beam.hip -- verse-constrained CTC prefix beam search on log-probs already in HBM (include/qverse.h: qv_beam_decode,
// qv_beam_batch; the trie: qv_trie_host.h).
//
// Every hypothesis is a node of the trie of the verse token sequences, so a prefix needs no string: a hypothesis is
// (node, pb, pnb) and at most two contributions meet in one candidate node -- the hypothesis already there ("stay") and its
// parent's extension.  k_trie_beam runs one workgroup per utterance; per frame
//   wave 0        finds, for every hypothesis, its parent among the (at most 64) hypotheses and which of them are its
//                 children (a child's number lies in [first_child, first_child + n_child)), and the prefix sum over
//                 1 + n_child that enumerates the candidates;
//   all threads   evaluate the candidates in chunks of 256 (candidate j -> hypothesis by binary search in the prefix sums;
//                 slot 0 = stay, slot s = child s - 1, whose record is the one 8-byte load from HBM; a child that is itself in
//                 the beam is folded into that hypothesis' stay and not counted twice) and rank the chunk together with the
//                 best W so far: an item's rank is the number of items ahead of it in (total descending, node ascending);
//                 ranks below W are the new best W.  No candidate count is too large: a frame just takes more chunks.
// The frame row (1025 floats) is staged in LDS; the next row is requested before the current one is processed and stored
// after it.  All score arithmetic is float64 in the order the header documents; frames t >= t_host[b] are never read.
#include "qv_rows.h"
#include "qv_trie_host.h"

namespace {

#define BM_THREADS 256
#define BM_W QV_BEAM_MAX
#define BM_POOL (BM_W + BM_THREADS)
#define BM_ROW_LOADS ((QV_VOCAB + BM_THREADS - 1) / BM_THREADS)
#define BM_NONE 0xFFFFFFFFu

struct BeamOut { int32_t node, pad; double score, pb, pnb; };
static_assert(sizeof(BeamOut) == 32 && sizeof(qv_beam_info) == 16, "record layout");
#define BM_ROW_BYTES (sizeof(qv_beam_info) + BM_W * sizeof(BeamOut))

__device__ __forceinline__ double bm_lae(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double hi = a >= b ? a : b, lo = a >= b ? b : a;
    return hi + log1p(exp(lo - hi));
}

__global__ __launch_bounds__(BM_THREADS) void k_trie_beam(const float *__restrict__ lp, int t_max, const int32_t *__restrict__ t_dev,
                                                          const QvTrieRec *__restrict__ trie, uint32_t n_nodes, int W,
                                                          unsigned char *__restrict__ out) {
    __shared__ float s_row[2][BM_ROW_LOADS * BM_THREADS];
    // the beam, best first
    __shared__ uint32_t b_node[BM_W], b_fc[BM_W];
    __shared__ uint16_t b_nc[BM_W], b_tok[BM_W];
    __shared__ double b_pb[BM_W], b_pnb[BM_W], b_tot[BM_W];
    __shared__ int b_par[BM_W], b_off[BM_W + 1];
    __shared__ unsigned long long b_kid[BM_W];
    // slots 0 .. BM_W - 1: the best so far of this frame; BM_W ..: the chunk under evaluation (node BM_NONE: no candidate)
    __shared__ double p_tot[BM_POOL], p_pb[BM_POOL], p_pnb[BM_POOL];
    __shared__ uint32_t p_node[BM_POOL], p_fc[BM_POOL];
    __shared__ uint16_t p_nc[BM_POOL], p_tok[BM_POOL];
    // ... and where the ranks put the next best W
    __shared__ double k_tot[BM_W], k_pb[BM_W], k_pnb[BM_W];
    __shared__ uint32_t k_node[BM_W], k_fc[BM_W];
    __shared__ uint16_t k_nc[BM_W], k_tok[BM_W];

    const int b = blockIdx.x, tid = threadIdx.x;
    int T = t_dev[b];
    T = T < 0 ? 0 : T;
    T = T > t_max ? t_max : T;
    const float *rows = lp + (size_t)b * t_max * QV_VOCAB;

    if (tid == 0) {
        const QvTrieRec r = trie[0];
        b_node[0] = 0; b_fc[0] = r.first_child; b_nc[0] = r.n_child; b_tok[0] = 0;
        b_pb[0] = 0.0; b_pnb[0] = -INFINITY; b_tot[0] = 0.0;
    }
    if (T > 0)
        for (int q = 0; q < BM_ROW_LOADS; ++q) {
            const int i = tid + q * BM_THREADS;
            s_row[0][i] = i < QV_VOCAB ? rows[i] : -INFINITY;
        }
    int nb = 1, max_cand = 0;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        const float *row = s_row[t & 1];
        // the next row is requested now and stored behind this frame's work
        float nxt[BM_ROW_LOADS];
        const bool more = t + 1 < T;
        if (more) {
            const float *g = rows + (size_t)(t + 1) * QV_VOCAB;
#pragma unroll
            for (int q = 0; q < BM_ROW_LOADS; ++q) {
                const int i = tid + q * BM_THREADS;
                nxt[q] = i < QV_VOCAB ? g[i] : -INFINITY;
            }
        }
        // ---- wave 0: parents, children in the beam, candidate enumeration
        if (tid < 64) {
            const bool live = tid < nb;
            const uint32_t my_node = live ? b_node[tid] : 0u, my_fc = live ? b_fc[tid] : 0u, my_nc = live ? b_nc[tid] : 0u;
            int par = -1;
            unsigned long long kid = 0ull;
            if (live)
                for (int j = 0; j < nb; ++j) {
                    if (b_node[j] - my_fc < my_nc) kid |= 1ull << j;
                    if (my_node - b_fc[j] < (uint32_t)b_nc[j]) par = j;
                }
            int cnt = live ? 1 + (int)my_nc : 0, incl = cnt, dup = __popcll(kid);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o);
                if (tid >= o) incl += v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dup += __shfl_xor(dup, o);
            if (live) { b_par[tid] = par; b_kid[tid] = kid; b_off[tid] = incl - cnt; }
            const int total = __shfl(incl, 63);
            if (tid == 0) b_off[BM_W] = total;
            max_cand = max(max_cand, total - dup);   // distinct candidate nodes of this frame
        }
        __syncthreads();
        const int C = b_off[BM_W];
        const double lb = (double)row[QV_BLANK];
        int nk = 0;   // entries in the pool's kept slots
        for (int base = 0; base < C; base += BM_THREADS) {
            // ---- one candidate per thread
            const int j = base + tid;
            uint32_t node = BM_NONE, fc = 0;
            uint16_t nc = 0, tk = 0;
            double pb = -INFINITY, pnb = -INFINITY, tot = -INFINITY;
            if (j < C) {
                int lo = 0, hi = nb - 1;   // the last hypothesis whose first candidate is at or before j
                while (lo < hi) {
                    const int m = (lo + hi + 1) >> 1;
                    if (b_off[m] <= j) lo = m; else hi = m - 1;
                }
                const int i = lo, slot = j - b_off[i];
                const uint32_t n_i = b_node[i];
                const uint16_t tok_i = b_tok[i];
                if (slot == 0) {   // stay, and the parent's extension into this node when the parent is in the beam
                    node = n_i; fc = b_fc[i]; nc = b_nc[i]; tk = tok_i;
                    pb = b_tot[i] + lb;
                    const double s = n_i == 0 ? -INFINITY : b_pnb[i] + (double)row[tok_i];
                    double x = -INFINITY;
                    const int p = b_par[i];
                    if (p >= 0) x = ((b_node[p] != 0 && tok_i == b_tok[p]) ? b_pb[p] : b_tot[p]) + (double)row[tok_i];
                    pnb = bm_lae(s, x);
                } else {
                    const uint32_t c = b_fc[i] + (uint32_t)(slot - 1);
                    bool in_beam = false;
                    for (unsigned long long m = b_kid[i]; m; m &= m - 1) in_beam = in_beam || b_node[__ffsll((long long)m) - 1] == c;
                    if (!in_beam && c < n_nodes) {
                        const QvTrieRec r = trie[c];
                        node = c; fc = r.first_child; nc = r.n_child; tk = r.tok;
                        pnb = ((n_i != 0 && tk == tok_i) ? b_pb[i] : b_tot[i]) + (double)row[tk];
                    }
                }
                tot = bm_lae(pb, pnb);
                if (tot == -INFINITY) node = BM_NONE;   // dropped
            }
            const int ps = BM_W + tid;
            p_node[ps] = node; p_fc[ps] = fc; p_nc[ps] = nc; p_tok[ps] = tk;
            p_pb[ps] = pb; p_pnb[ps] = pnb; p_tot[ps] = tot;
            const int n_new = __syncthreads_count(node != BM_NONE);
            // ---- rank the chunk and the best so far together: (total descending, node ascending) is a strict order
            const int n_chunk = min(BM_THREADS, C - base);
            for (int pass = 0; pass < 2; ++pass) {
                const int me = pass == 0 ? ps : tid;
                if (pass == 1 && tid >= nk) break;
                const uint32_t my_node = p_node[me];
                if (my_node == BM_NONE) continue;
                const double my_tot = p_tot[me];
                int rank = 0;
                for (int q = 0; q < nk; ++q) rank += (p_tot[q] > my_tot || (p_tot[q] == my_tot && p_node[q] < my_node)) ? 1 : 0;
                for (int q = BM_W; q < BM_W + n_chunk; ++q) rank += (p_tot[q] > my_tot || (p_tot[q] == my_tot && p_node[q] < my_node)) ? 1 : 0;
                if (rank < W) {
                    k_node[rank] = my_node; k_fc[rank] = p_fc[me]; k_nc[rank] = p_nc[me]; k_tok[rank] = p_tok[me];
                    k_pb[rank] = p_pb[me]; k_pnb[rank] = p_pnb[me]; k_tot[rank] = my_tot;
                }
            }
            __syncthreads();
            nk = min(W, nk + n_new);
            if (tid < nk) {
                p_node[tid] = k_node[tid]; p_fc[tid] = k_fc[tid]; p_nc[tid] = k_nc[tid]; p_tok[tid] = k_tok[tid];
                p_pb[tid] = k_pb[tid]; p_pnb[tid] = k_pnb[tid]; p_tot[tid] = k_tot[tid];
            }
            __syncthreads();
        }
        // ---- the best W of the frame are the next beam, already in order
        nb = nk;
        if (tid < nb) {
            b_node[tid] = p_node[tid]; b_fc[tid] = p_fc[tid]; b_nc[tid] = p_nc[tid]; b_tok[tid] = p_tok[tid];
            b_pb[tid] = p_pb[tid]; b_pnb[tid] = p_pnb[tid]; b_tot[tid] = p_tot[tid];
        }
        if (more) {
            float *dst = s_row[(t + 1) & 1];
#pragma unroll
            for (int q = 0; q < BM_ROW_LOADS; ++q) dst[tid + q * BM_THREADS] = nxt[q];
        }
        __syncthreads();
    }

    unsigned char *rec = out + (size_t)b * BM_ROW_BYTES;
    if (tid == 0) {
        qv_beam_info inf;
        inf.n_entries = nb; inf.t_frames = T; inf.max_candidates = max_cand; inf.reserved = 0;
        *(qv_beam_info *)rec = inf;
    }
    if (tid < BM_W) {
        BeamOut o;
        const bool live = tid < nb;
        o.node = live ? (int32_t)b_node[tid] : -1; o.pad = 0;
        o.score = live ? b_tot[tid] : 0.0; o.pb = live ? b_pb[tid] : 0.0; o.pnb = live ? b_pnb[tid] : 0.0;
        ((BeamOut *)(rec + sizeof(qv_beam_info)))[tid] = o;
    }
}

}  // namespace

// What the engine keeps for the search: the trie of the span last asked for (host arrays; `rec` also in HBM) and the host copy
// of the token table it is built from.
struct QvBeamState {
    QvTrie trie;
    QvTrieRec *rec_dev = nullptr;
    std::vector<uint32_t> tok_off;
    std::vector<uint16_t> tok;
};

void qv_beam_free(qv_engine *eng) {
    if (!eng->beam) return;
    if (eng->beam->rec_dev) (void)hipFree(eng->beam->rec_dev);
    delete eng->beam;
    eng->beam = nullptr;
}

// the trie for `max_span`, built and uploaded by the first call that asks for it, kept until another span is asked for
int qv_beam_trie(qv_engine *eng, int max_span, const QvTrie **out) {
    if (max_span < 1 || max_span > QV_TRIE_MAX_SPAN) { qv_set_error(eng, "beam search: max_span outside 1..6"); return QV_ERR_ARG; }
    if (!eng->beam) eng->beam = new QvBeamState();
    QvBeamState &s = *eng->beam;
    if (s.rec_dev && s.trie.max_span == max_span) { *out = &s.trie; return QV_OK; }
    if (s.tok_off.empty()) {   // the token table back from HBM, where qv_create left it
        const size_t NK = (size_t)eng->tab.n_verses * QV_MAX_SPAN;
        std::vector<uint32_t> off(NK + 1);
        QV_HIP(hipMemcpy(off.data(), eng->tab.tok_off, sizeof(uint32_t) * (NK + 1), hipMemcpyDeviceToHost));
        std::vector<uint16_t> tok(off[NK]);
        if (off[NK]) QV_HIP(hipMemcpy(tok.data(), eng->tab.tok, sizeof(uint16_t) * off[NK], hipMemcpyDeviceToHost));
        s.tok_off.swap(off);
        s.tok.swap(tok);
    }
    if (s.rec_dev) {   // (beam calls are synchronous: no launch still reads the trie that is replaced)
        (void)hipFree(s.rec_dev);
        s.rec_dev = nullptr;
    }
    std::string err;
    const int rc = qv_trie_build(eng->tab.n_verses, s.tok_off.data(), s.tok_off.size(), s.tok.data(), s.tok.size(), max_span, s.trie, err);
    if (rc) { s.trie = QvTrie(); qv_set_error(eng, err); return rc == QV_TRIE_BAD_ARG ? QV_ERR_ARG : QV_ERR_IO; }
    void *d = nullptr;
    const size_t bytes = s.trie.n_nodes() * sizeof(QvTrieRec);
    if (hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); s.trie = QvTrie(); qv_set_error(eng, "beam search: no memory for the trie"); return QV_ERR_HIP; }
    s.rec_dev = (QvTrieRec *)d;
    QV_HIP(hipMemcpy(d, s.trie.rec.data(), bytes, hipMemcpyHostToDevice));
    *out = &s.trie;
    return QV_OK;
}

int qv_beam_node_tokens(qv_engine *eng, int max_span, int node, int32_t *ids_out, int cap, int32_t *n_out) {
    const QvTrie *t = nullptr;
    int rc = qv_beam_trie(eng, max_span, &t);
    if (rc) return rc;
    std::vector<uint16_t> ids;
    if (node < 0 || !qv_trie_node_tokens(*t, (uint32_t)node, ids)) { qv_set_error(eng, "qv_trie_node_tokens: no such node"); return QV_ERR_ARG; }
    if ((int)ids.size() > cap) { qv_set_error(eng, "qv_trie_node_tokens: the node has more tokens than `cap`"); return QV_ERR_ARG; }
    for (size_t i = 0; i < ids.size(); ++i) ids_out[i] = ids[i];
    *n_out = (int32_t)ids.size();
    return QV_OK;
}

// frame counts up, kernel, one copy back, the records completed from the host trie; SYNCHRONOUS on `stream`.  The workspace
// of the context, allocated by the first call that uses it: per row of max_batch the frame count going up and one record
// coming back (16 + 64 * 32 bytes).
int qv_beam_rows(qv_engine *eng, QvCtx &c, const float *lp, const int32_t *t_host, int batch, int t_max, int max_span, int W, int k,
                 qv_beam_info *info_host, qv_beam_entry *entries_host, int32_t *ids_host, int pitch, hipStream_t stream) {
    QV_TRY_RC(qv_rows_check(eng, "beam search", c, batch, t_max, t_host));
    const QvTrie *trie = nullptr;
    QV_TRY_RC(qv_beam_trie(eng, max_span, &trie));
    QvRowWs &w = c.beam;
    QV_TRY_RC(qv_row_ws(eng, c, w, BM_ROW_BYTES, "beam workspace"));
    QV_TRY_RC(qv_rows_send_t(eng, w, t_host, batch, stream));
    hipLaunchKernelGGL(k_trie_beam, dim3(batch), dim3(BM_THREADS), 0, stream, lp, t_max, (const int32_t *)w.m.dev,
                       (const QvTrieRec *)eng->beam->rec_dev, (uint32_t)trie->n_nodes(), W, w.m.dev + w.t_bytes);
    QV_HIP(hipGetLastError());
    QV_TRY_RC(qv_fetch_sync(eng, w.m.host + w.t_bytes, w.m.dev + w.t_bytes, BM_ROW_BYTES * batch, stream));
    std::vector<uint16_t> ids;
    for (int b = 0; b < batch; ++b) {
        const unsigned char *rec = w.m.host + w.t_bytes + BM_ROW_BYTES * b;
        qv_beam_info inf;
        memcpy(&inf, rec, sizeof inf);
        const BeamOut *o = (const BeamOut *)(rec + sizeof(qv_beam_info));
        inf.n_entries = inf.n_entries < k ? inf.n_entries : k;
        info_host[b] = inf;
        for (int e = 0; e < k; ++e) {
            qv_beam_entry &d = entries_host[(size_t)b * k + e];
            memset(&d, 0, sizeof d);
            if (e >= inf.n_entries) continue;
            const uint32_t n = (uint32_t)o[e].node;
            if (n >= trie->n_nodes()) { qv_set_error(eng, "beam search: the kernel reported a node outside the trie"); return QV_ERR_HIP; }
            const uint32_t e0 = trie->end_off[n], e1 = trie->end_off[n + 1];
            d.node = (int32_t)n;
            d.n_tokens = trie->depth[n];
            d.n_ends = (int32_t)(e1 - e0);
            d.start_verse = -1;
            if (e1 > e0) {
                const QvTrieEnd &f = trie->ends[e0];
                d.start_verse = f.verse; d.span = f.span;
                d.surah = eng->h_surah[f.verse]; d.ayah = eng->h_ayah[f.verse]; d.ayah_end = d.ayah + f.span - 1;
                d.flags = QV_BEAM_COMPLETE;
            }
            d.below_count = (int32_t)trie->below_count[n];
            d.below_verse = trie->below_first[n].verse;
            d.below_span = trie->below_first[n].span;
            d.score = o[e].score; d.blank_score = o[e].pb; d.nonblank_score = o[e].pnb;
        }
        if (ids_host) {
            int32_t *row = ids_host + (size_t)b * pitch;
            int n = 0;
            if (inf.n_entries > 0 && qv_trie_node_tokens(*trie, (uint32_t)o[0].node, ids)) {
                n = (int)ids.size() < pitch ? (int)ids.size() : pitch;
                for (int i = 0; i < n; ++i) row[i] = ids[i];
            }
            for (int i = n; i < pitch; ++i) row[i] = -1;
        }
    }
    return QV_OK;
}
