// qv_lcs.h -- the bit-parallel LCS core (Indel distance) of the matching kernels: one text per lane (lcs_chunk .. lcs_dispatch),
// the pattern's words spread over neighbouring lanes (lcs_systolic, lcs_systolic_chunks for the prefix-shared span pass) and
// the LDS copy of a transcript's match masks (load_pm_lds).  Parameterised by the matching window through QV_MAXW, which only
// qv_match_body.inc defines: nothing else includes this file.
#pragma once
#include "qv_limits.h"   // QV_NSYM, QV_MAX_VW

#ifndef QV_LCS_ADDC
#define QV_LCS_ADDC 1   // 0: the compiler's own carry chain (cross-check builds)
#endif
// ------------------------------------------------------------------ bit-parallel LCS ---
// Hyyro/Crochemore: V all ones; per text char U = V & M; V = (V + U) | (V & ~M).
// pm: match masks [sym][stride] (u64), W words used; text codes >= QV_NSYM match nothing.
// lcs_chunk advances the recurrence over the first cnt (<= 8) codes packed in `chunk`; lcs_feed continues it over n
// more text codes (V carries the state); lcs_count reads the LCS length of everything fed so far: LCS(pattern, text[:j]) is
// available at every j of one walk over the text.
// 64-bit a + b + carry-in -> sum, carry-out, with the carry held as a LANE MASK in an SGPR pair (v_addc_co_u32's VOP3 form takes any
// pair as carry source and destination): two instructions per word.  The generic lowering of __builtin_addcll costs two 64-bit
// adds, two 64-bit compares and the selects that turn them into a carry value -- the window scans, the full-string pass and the
// span pass are bound by VALU issue (profiles/r06_c_pmc_post.txt: 202 M / 82 M / 118 M VALU instructions per launch), and the carry
// was half of a word-step's instructions.
static __device__ __forceinline__ uint64_t addc64(uint64_t a, uint64_t b, unsigned long long &carry) {
    uint32_t lo, hi;
    asm("v_addc_co_u32 %0, %2, %3, %4, %2\n\tv_addc_co_u32 %1, %2, %5, %6, %2"
        : "=&v"(lo), "=&v"(hi), "+s"(carry)
        : "v"((uint32_t)a), "v"((uint32_t)b), "v"((uint32_t)(a >> 32)), "v"((uint32_t)(b >> 32)));
    return ((uint64_t)hi << 32) | lo;
}

// ZROW: the mask table has an all-zero row at index QV_NSYM (the LDS copies: load_pm_lds, k_frag's slice): codes past cnt
// and codes outside the alphabet select THAT row, instead of a select per mask word (2 of a word-step's ~10 instructions).
template <int W, bool ZROW = false>
static __device__ __forceinline__ void lcs_chunk(uint64_t (&V)[W], const uint64_t *__restrict__ pm, int stride, uint64_t chunk, int cnt) {
    // The match masks of CH consecutive codes are requested TOGETHER, before the dependent add chain
    // of those steps: the recurrence is one serial chain per lane, and a mask load inside every step
    // (L1/L2 or LDS latency each) used to be most of a step's time.  Codes past cnt
    // and codes outside the alphabet get an all-zero mask, which leaves V unchanged.
    constexpr int CH = W <= 4 ? 8 : (W <= 8 ? 4 : 1);   // (wider patterns: fewer masks in flight -- mk[CH][W] sets the kernels' VGPR count, i.e. how many waves a SIMD interleaves)
#pragma unroll
    for (int g0 = 0; g0 < 8; g0 += CH) {
        if (g0 >= cnt) break;
        uint64_t mk[CH][W];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            int c = (int)((chunk >> (8 * (g0 + e))) & 0xFF);
            const bool valid = g0 + e < cnt && c < QV_NSYM;
            const uint64_t *M = pm + (size_t)(valid ? c : (ZROW ? QV_NSYM : 0)) * stride;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t x = M[w];
                mk[e][w] = (ZROW || valid) ? x : 0ull;
            }
        }
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            unsigned long long carry = 0;   // lane mask of the carries (addc64)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t v = V[w], mm = mk[e][w];
                // v + (v & mm) + carry with the carry chained through the words
                uint64_t s2 = QV_LCS_ADDC ? addc64(v, v & mm, carry) : __builtin_addcll(v, v & mm, carry, &carry);
                V[w] = s2 | (v & ~mm);
            }
        }
    }
}

typedef uint64_t __attribute__((aligned(1))) u64_unaligned;

template <int W, bool ZROW = false>
static __device__ __forceinline__ void lcs_feed(uint64_t (&V)[W], const uint64_t *__restrict__ pm, int stride,
                                         const uint8_t *__restrict__ text, int n) {
    // the text is fetched 8 codes per (possibly unaligned) load: one memory access per 8 steps
    // of the recurrence instead of one per step; every text buffer is padded by >= 8 bytes
    // ... and the NEXT 8 codes are requested before this chunk's steps run: the lane's chain used to start every chunk
    // with an exposed global-load latency, and a kernel lasts as long as its longest text (1,100+ codes = 140 chunks)
    uint64_t next = n > 0 ? *(const u64_unaligned *)text : 0ull;
    for (int j0 = 0; j0 < n; j0 += 8) {
        const uint64_t chunk = next;
        if (j0 + 8 < n) next = *(const u64_unaligned *)(text + j0 + 8);
        lcs_chunk<W, ZROW>(V, pm, stride, chunk, n - j0 < 8 ? n - j0 : 8);
    }
}

template <int W>
static __device__ __forceinline__ int lcs_count(const uint64_t (&V)[W], int m) {
    int zeros = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint64_t z = ~V[w];
        int lo = w * 64;
        if (m < lo + 64) z &= (m > lo) ? ((1ull << (m - lo)) - 1ull) : 0ull;
        zeros += __popcll(z);
    }
    return zeros;
}

template <int W, bool ZROW = false>
static __device__ __forceinline__ int lcs_core(const uint64_t *__restrict__ pm, int stride, const uint8_t *__restrict__ text,
                                        int n, int m) {
    uint64_t V[W];
#pragma unroll
    for (int w = 0; w < W; ++w) V[w] = ~0ull;
    lcs_feed<W, ZROW>(V, pm, stride, text, n);
    return lcs_count<W>(V, m);
}

// WMAX: the longest pattern the call site can have.  Verse texts are at most QV_MAX_VW words, so only the sites whose
// pattern is the TRANSCRIPT instantiate the 24- and 32-word cores of the wide window (V[W] and one step's W mask words
// live in VGPRs: 64 + 64 registers at 32 words, CH = 1; the kernel's register count is that of its widest core).
template <bool ZROW = false, int WMAX = QV_MAXW>
static __device__ __forceinline__ int lcs_dispatch(int W, const uint64_t *pm, int stride, const uint8_t *text, int n, int m) {
    if (n <= 0 || m <= 0) return 0;
    if (W <= 1) return lcs_core<1, ZROW>(pm, stride, text, n, m);
    if (W <= 2) return lcs_core<2, ZROW>(pm, stride, text, n, m);
    if (W <= 3) return lcs_core<3, ZROW>(pm, stride, text, n, m);
    if (W <= 4) return lcs_core<4, ZROW>(pm, stride, text, n, m);
    if (W <= 6) return lcs_core<6, ZROW>(pm, stride, text, n, m);
    if (W <= 8) return lcs_core<8, ZROW>(pm, stride, text, n, m);
    if (W <= 11) return lcs_core<11, ZROW>(pm, stride, text, n, m);
#if QV_MAXW > 16
    if constexpr (WMAX > 16) {
        if (W <= 16) return lcs_core<16, ZROW>(pm, stride, text, n, m);
        if (W <= 24) return lcs_core<24, ZROW>(pm, stride, text, n, m);
        return lcs_core<32, ZROW>(pm, stride, text, n, m);
    }
#endif
    return lcs_core<16, ZROW>(pm, stride, text, n, m);
}

// ---- the same recurrence with the pattern's words spread over G neighbouring lanes (G = 4, 8, 16; lane w of the group
// owns word w) as a skewed wavefront: at step t lane w applies text code j = t - w, with the carry lane w - 1 produced for
// that code one step earlier (one DPP row shift).  A lane's serial chain is then one 64-bit add per text code instead of
// W of them: the span pass and the window scans last as long as their LONGEST lane, and for transcripts of several hundred
// characters (W = 4..7) that lane used to walk 1,000+ codes x W words.  Same integer result as lcs_core.
// All G lanes pass the same text / n / m / W; the return value is valid in every lane of the group.
// G = 32 (wide window, 17..32 words): row_shr:1 stops at the 16-lane DPP row, so lane 16 of a group would never see lane
// 15's carry; there the carry moves with a wave-wide shuffle (ds_bpermute_b32) -- lcs_carry_in.
template <int G>
static __device__ __forceinline__ unsigned lcs_carry_in(unsigned cout) {
#if QV_MAXW > 16
    if constexpr (G > 16) return (unsigned)__shfl_up((int)cout, 1);
#endif
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)cout, 0x111 /* row_shr:1 */, 0xF, 0xF, true);
}
template <int G>
static __device__ __forceinline__ int lcs_systolic(const uint64_t *__restrict__ pm, int stride, const uint8_t *__restrict__ text, int n,
                                            int m, int W, int w) {
    uint64_t V = ~0ull;
    unsigned cout = 0;                      // the carry this lane produced in its last step
    const bool act = w < W;
    const int total = n + G - 1;            // steps t = 0 .. total - 1; lane w is at code j = t - w
    for (int t0 = 0; t0 < total; t0 += 8) {
        const int j0 = t0 - w;
        uint64_t chunk = 0;                 // the lane's next 8 codes (text buffers are padded by >= 8 bytes)
        if (j0 < n && j0 > -8) chunk = j0 >= 0 ? *(const u64_unaligned *)(text + j0) : (*(const u64_unaligned *)text << (8 * -j0));
        uint64_t mk[8];                     // their match-mask words, requested together in front of the dependent chain
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + e, c = (int)((chunk >> (8 * e)) & 0xFF);
            const bool valid = act && j >= 0 && j < n && c < QV_NSYM;
            const uint64_t x = pm[(size_t)(valid ? c : 0) * stride + (act ? w : 0)];
            mk[e] = valid ? x : 0ull;       // a zero mask leaves V alone and produces no carry
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            unsigned cin = lcs_carry_in<G>(cout);
            if (w == 0) cin = 0;
            unsigned long long carry;
            const uint64_t s2 = __builtin_addcll(V, V & mk[e], (unsigned long long)cin, &carry);
            V = s2 | (V & ~mk[e]);
            cout = (unsigned)carry;
        }
    }
    uint64_t z = ~V;
    const int lo = w * 64;
    if (m < lo + 64) z &= (m > lo) ? ((1ull << (m - lo)) - 1ull) : 0ull;
    int cnt = act ? __popcll(z) : 0;
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    return cnt;
}

// stage the transcript's match masks (both the spaced and the spaceless pattern, 10 KB) in LDS
// LDS row stride of the match masks (u64 units).  With the global stride QV_MAXW = 16 (128 B) every
// symbol's word w sat in the same two banks, so the 64 lanes of a wave - each on a different
// symbol - serialised their mask reads; the padded stride spreads the rows over the banks.
#ifndef QV_PMS
#define QV_PMS (QV_MAXW + 2)   // 144 B rows: 16-byte aligned for ds_read_b128, 16 distinct bank offsets
#endif
#define QV_PM_ROWS (QV_NSYM + 1)   // rows per pattern of an LDS copy: the alphabet + one all-zero row (lcs_chunk<W, true>)
static __device__ __forceinline__ void load_pm_lds(uint64_t *spm, const uint64_t *gpm) {
    for (int i = threadIdx.x; i < 2 * QV_NSYM * QV_MAXW; i += blockDim.x) {
        const int row = i / QV_MAXW, p = row / QV_NSYM;
        spm[(p * QV_PM_ROWS + row - p * QV_NSYM) * QV_PMS + (i % QV_MAXW)] = gpm[i];
    }
    for (int i = threadIdx.x; i < 2 * QV_PMS; i += blockDim.x) spm[((i / QV_PMS) * QV_PM_ROWS + QV_NSYM) * QV_PMS + (i % QV_PMS)] = 0ull;
    __syncthreads();
}

struct SpanJob {
    int v0, emax;              // start verse; longest span (in ayat) that survives the bound, 0 = none
    unsigned surv;             // bit e: the span of e ayat survives
    uint32_t start;            // its text in tab.clean
    uint32_t a0;               // first chunk in tab.clean8 (multiple of 8)
    int lead;                  // codes of that chunk in front of the text
    double bonus;
    unsigned long long key0;   // tie-break key of the span of 2 ayat (the span of e: key0 + e - 2)
};

// the pattern's words spread over G lanes as in lcs_systolic, but skewed by whole CHUNKS: at chunk-step t lane w runs the
// 8 codes of chunk t - w with the 8 carries lane w - 1 produced for that chunk one step earlier (one DPP per chunk instead
// of one per code; every lane is chunk-aligned, so "an ayah ends here" is one compare per chunk).  snap packs the lane's
// zero counts at the ends of ayat 2 .. (7 bits each); all G lanes pass the same job.
template <int G>
static __device__ __forceinline__ uint64_t lcs_systolic_chunks(const uint64_t *__restrict__ pm, int stride, const uint8_t *__restrict__ c8,
                                                        const uint32_t *__restrict__ off8, const SpanJob &j, int m, int W, int w) {
    uint64_t V = ~0ull, snap = 0;
    unsigned cout8 = 0;
    const bool act = w < W;
    const int lo = w * 64;
    const uint64_t zmask = !act ? 0ull : (m >= lo + 64 ? ~0ull : (m > lo ? ((1ull << (m - lo)) - 1ull) : 0ull));
    const int nch = (int)(off8[j.v0 + j.emax] - j.a0) >> 3;
    int e = 1, next_end = (int)(off8[j.v0 + 1] - j.a0) >> 3;       // chunks up to the end of ayah e
    for (int t = 0; t < nch + G - 1; ++t) {
        const int c = t - w;
        unsigned cin8 = lcs_carry_in<G>(cout8);   // (G = 32: one shuffle per CHUNK of 8 codes)
        if (w == 0) cin8 = 0;
        uint64_t chunk = ~0ull;                 // filler: matches nothing
        if (c >= 0 && c < nch) chunk = *(const uint64_t *)(c8 + j.a0 + 8 * (size_t)c);
        if (c == 0 && j.lead) chunk |= (1ull << (8 * j.lead)) - 1ull;
        uint64_t mk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int code = (int)((chunk >> (8 * k)) & 0xFF);
            const bool valid = act && code < QV_NSYM;
            // (pm is always load_pm_lds's copy here: invalid codes and idle lanes read its all-zero row -- a zero mask leaves V
            // alone and produces no carry)
            mk[k] = pm[(size_t)(valid ? code : QV_NSYM) * stride + (act ? w : 0)];
        }
        cout8 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            unsigned long long carry;
            const uint64_t s2 = __builtin_addcll(V, V & mk[k], (unsigned long long)((cin8 >> k) & 1u), &carry);
            V = s2 | (V & ~mk[k]);
            cout8 |= (unsigned)carry << k;
        }
        if (c + 1 == next_end) {                // the ayah ends with this chunk (rare: <= max_span times per walk)
            if (e >= 2) snap |= (uint64_t)__popcll(~V & zmask) << (7 * (e - 2));
            ++e;
            // (past the longest surviving span nothing is read off any more: the skewed lanes keep stepping for up to G - 1
            // chunks after the walk's last one, and further ayah ends there must not shift into the fields above)
            next_end = e <= j.emax ? (int)(off8[j.v0 + e] - j.a0) >> 3 : 0x7FFFFFFF;
        }
    }
    return snap;
}
