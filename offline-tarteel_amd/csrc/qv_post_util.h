// qv_post_util.h -- stateless device helpers that both the once-compiled post-logits kernels (qv_postlogits.hip) and the
// per-window matching kernels (qv_match_body.inc) use: the Indel ratio, wave / block reductions, the stable top-k selection,
// CPython's set order, the verse text variants and round(x, 3).  Nothing here mentions the matching window.
#pragma once
#include "qv_common.h"
#include "qv_greedy.h"   // better()

static __device__ __forceinline__ double ratio_from(int lcs, int la, int lb) {
    int tot = la + lb;
    if (tot == 0) return 1.0;
    return __dsub_rn(1.0, __ddiv_rn((double)(tot - 2 * lcs), (double)tot));
}

static __device__ __forceinline__ int wave_rank(bool pred, int lane, int &total) {
    unsigned long long m = __ballot(pred);
    total = __popcll(m);
    return __popcll(m & ((1ull << lane) - 1ull));
}

static __device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
static __device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (better(): the (score desc, key asc) ordering of every stable "sorted(..., reverse=True)" emulation -- qv_greedy.h)
static __device__ __forceinline__ void wave_best(double &s, unsigned long long &k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        double s2 = __shfl_xor(s, o);
        unsigned long long k2 = __shfl_xor(k, o);
        if (better(s2, k2, s, k)) { s = s2; k = k2; }
    }
}

// block-wide best over 256 threads; result valid in all threads.  sh_s/sh_k: [4+1] scratch.
static __device__ __forceinline__ void block_best(double &s, unsigned long long &k, double *sh_s, unsigned long long *sh_k) {
    wave_best(s, k);
    int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh_s[w] = s; sh_k[w] = k; }
    __syncthreads();
    s = sh_s[0]; k = sh_k[0];
    for (int i = 1; i < nw; ++i)
        if (better(sh_s[i], sh_k[i], s, k)) { s = sh_s[i]; k = sh_k[i]; }
}

// best non-negative entry among the positions p = tid, tid + 256, ... that this thread owns.
// Top-k selection keeps each thread's best cached: after a round only the owner of the winner
// rescans its ~25 entries, so a round costs one block reduction instead of a full scan.
static __device__ __forceinline__ void local_best(const double *sc, int n, int tid, double &s, unsigned long long &k) {
    s = -1.0;
    k = ~0ull;
    for (int p = tid; p < n; p += 256) {
        double x = sc[p];
        if (x >= 0.0 && better(x, (unsigned long long)p, s, k)) { s = x; k = p; }
    }
}

// Top-K of sc[0..n) (entries < 0 excluded) in the order of a stable descending sort, i.e.
// (score desc, position asc), for a 256-thread block.  MSB-first radix select on the
// order-preserving bit pattern of the non-negative doubles finds the K-th largest value in 8
// histogram passes; ties at that value are taken in position order; the <= K survivors are
// ordered by rank counting.  scratch: u32[256 + 8], sel_p: i32[K], sel_s: f64[K] (LDS).
// out_p / out_s may be global.  Returns the number selected (same in every thread).
static __device__ int block_topk_select(const double *sc, int n, int K, uint32_t *scratch, int32_t *sel_p, double *sel_s,
                                        int32_t *out_p, double *out_s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *hist = scratch, *misc = scratch + 256;  // misc: [0] digit, [1] need, [2] count, [3..6] wave sums
    auto key_of = [&](int p) -> unsigned long long {
        double x = sc[p];
        return x >= 0.0 ? (unsigned long long)__double_as_longlong(x) + 1ull : 0ull;
    };
    // number of valid entries
    int cnt = 0;
    for (int p = tid; p < n; p += 256) cnt += sc[p] >= 0.0;
    cnt = wave_sum_i(cnt);
    if (lane == 0) misc[3 + wave] = cnt;
    if (tid == 0) misc[2] = 0;
    __syncthreads();
    const int nvalid = misc[3] + misc[4] + misc[5] + misc[6];
    if (K > nvalid) K = nvalid;
    if (K <= 0) return 0;
    unsigned long long prefix = 0, mask = 0;
    int need = K;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        hist[tid] = 0;
        __syncthreads();
        for (int p = tid; p < n; p += 256) {
            unsigned long long k = key_of(p);
            if (k != 0 && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1u);
        }
        __syncthreads();
        if (wave == 0) {
            // bins 255..0: lane l owns bins 4l..4l+3; suffix sums from the top
            uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            uint32_t tot = h0 + h1 + h2 + h3, suf = tot;  // inclusive suffix over lanes >= l
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                uint32_t x = __shfl_down(suf, o);
                if (lane + o < 64) suf += x;
            }
            uint32_t above = suf - tot;  // elements in bins of higher lanes
            bool here = above < (uint32_t)need && suf >= (uint32_t)need;
            if (here) {
                uint32_t c = above;
                int d;
                if (c + h3 >= (uint32_t)need) d = 3;
                else { c += h3; if (c + h2 >= (uint32_t)need) d = 2; else { c += h2; if (c + h1 >= (uint32_t)need) d = 1; else { c += h1; d = 0; } } }
                misc[0] = 4 * lane + d;
                misc[1] = need - (int)c;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)misc[0] << shift;
        mask |= 0xFFull << shift;
        need = (int)misc[1];
    }
    const unsigned long long T = prefix;  // key of the K-th largest; `need` of the == T entries are taken
    // entries above T (unordered) ...
    for (int p = tid; p < n; p += 256) {
        unsigned long long k = key_of(p);
        if (k > T) { int slot = atomicAdd(&misc[2], 1u); sel_p[slot] = p; sel_s[slot] = sc[p]; }
    }
    // ... and the first `need` entries equal to T, in position order
    int taken = 0;
    for (int base = 0; base < n && taken < need; base += 256) {
        int p = base + tid;
        bool eq = p < n && key_of(p) == T;
        unsigned long long bal = __ballot(eq);
        int r = __popcll(bal & ((1ull << lane) - 1ull)), tot = __popcll(bal);
        __syncthreads();
        if (lane == 0) misc[3 + wave] = tot;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; ++w) before += misc[3 + w];
        int all = misc[3] + misc[4] + misc[5] + misc[6];
        if (eq && taken + before + r < need) { int slot = atomicAdd(&misc[2], 1u); sel_p[slot] = p; sel_s[slot] = sc[p]; }
        taken += all;
    }
    __syncthreads();
    // order the K survivors
    for (int i = tid; i < K; i += 256) {
        double si = sel_s[i];
        int pi = sel_p[i], rank = 0;
        for (int j = 0; j < K; ++j) rank += better(sel_s[j], (unsigned long long)sel_p[j], si, (unsigned long long)pi);
        out_p[rank] = pi;
        out_s[rank] = si;
    }
    __syncthreads();
    return K;
}

// CPython set[int] iteration order of ints inserted one by one (Objects/setobject.c: linear
// probes 9, perturb shift 5, x4 growth at fill*5 >= mask*3); match_verse iterates
// set(top-50) (quran_db.py:279-288) and sorts stably, so exact ties resolve in this order.
static __device__ int pyset_order(const int32_t *vals, int n, int32_t *out, int32_t *tabA, int32_t *tabB) {
    int mask = 7;
    int32_t *tab = tabA;
    for (int i = 0; i <= mask; ++i) tab[i] = -1;
    int fill = 0;
    for (int k = 0; k < n; ++k) {
        unsigned long long h = (unsigned long long)vals[k], perturb = h;
        int i = (int)(h & (unsigned)mask);
        int found = 0;
        for (;;) {
            int probes = (i + 9 <= mask) ? 9 : 0;
            int e = i;
            do {
                if (tab[e] < 0) { tab[e] = vals[k]; ++fill; found = 1; break; }
                if (tab[e] == vals[k]) { found = 2; break; }
                ++e;
            } while (probes--);
            if (found) break;
            perturb >>= 5;
            i = (int)(((unsigned long long)i * 5ull + 1ull + perturb) & (unsigned)mask);
        }
        if (found == 1 && fill * 5 >= mask * 3) {
            int minused = fill * 4, ns = 8;
            while (ns <= minused) ns <<= 1;
            int32_t *nt = (tab == tabA) ? tabB : tabA;
            for (int z = 0; z < ns; ++z) nt[z] = -1;
            int nmask = ns - 1;
            for (int z = 0; z <= mask; ++z) {
                if (tab[z] < 0) continue;
                unsigned long long hh = (unsigned long long)tab[z], pp = hh;
                int j = (int)(hh & (unsigned)nmask);
                for (;;) {
                    if (nt[j] < 0) { nt[j] = tab[z]; break; }
                    bool placed = false;
                    if (j + 9 <= nmask)
                        for (int q = 1; q <= 9; ++q)
                            if (nt[j + q] < 0) { nt[j + q] = tab[z]; placed = true; break; }
                    if (placed) break;
                    pp >>= 5;
                    j = (int)(((unsigned long long)j * 5ull + 1ull + pp) & (unsigned)nmask);
                }
            }
            tab = nt;
            mask = nmask;
        }
    }
    int c = 0;
    for (int z = 0; z <= mask; ++z)
        if (tab[z] >= 0) out[c++] = tab[z];
    return c;
}

struct TextRef { const uint8_t *p; int n; int nw; int tid; };

static __device__ __forceinline__ TextRef text_of(const QvTables &tab, int v, int variant) {
    TextRef t;
    if (variant == 0) { t.p = tab.clean + tab.clean_off[v]; t.n = tab.clean_len[v]; t.nw = tab.nw[0][v]; t.tid = v; }
    else if (variant == 1) { t.p = tab.alt + tab.alt_off[v]; t.n = tab.alt_len[v]; t.nw = tab.nw[1][v]; t.tid = tab.n_verses + v; }
    else {
        int nl = tab.nobsm_len[v];
        t.p = tab.clean + tab.clean_off[v] + tab.clean_len[v] - nl; t.n = nl; t.nw = tab.nw[2][v];
        t.tid = 2 * tab.n_verses + tab.nobsm_rank[v];
    }
    return t;
}

static __device__ __forceinline__ double py_round3(double x) {
    // round(x, 3) for x in [0, 1]: nearest k/1000 (ties cannot occur for non-representable
    // thousandths; exact halves x = (2k+1)/2000 are not binary fractions), then k/1000.0
    double y = __dmul_rn(x, 1000.0);
    double k = rint(y);
    // correct the (rare) case where x*1000 rounded across the .5 boundary
    double lo = __ddiv_rn(k - 0.5, 1000.0), hi = __ddiv_rn(k + 0.5, 1000.0);
    if (x < lo) k -= 1.0; else if (x > hi) k += 1.0;
    return __ddiv_rn(k, 1000.0);
}
