// qv_ctc_body.inc -- the CTC alpha recursion of the rerank: the two wave programs, the read-out and the kernel k_ctc<LONG, VAR>.
// Included INSIDE a namespace.  qv_postlogits.hip has it once for every engine (next to k_ctc_debug, the second caller of
// ctc_dispatch<true, *>, which is why the compiler keeps that function out of line there); qv_match_body.inc has it once
// more for the wide window's own k_ctc<true, *>, where the recursions are inlined into the kernel (DESIGN.md 4.19: the
// out-of-line form was measured 4 - 5 % slower on a wide engine with clips of more than 384 frames).

// ------------------------------------------------------------------ 9. CTC -------------
// ATen LossCTC.cpp float32 alpha recursion (what F.ctc_loss runs on CPU for the reference,
// c2c-direct/run.py:354-362).  One wave per target; state s = lane*NS + k.
template <int NS>
__device__ void ctc_wave(const float *__restrict__ lp, int T, const uint16_t *__restrict__ tgt, int L, int lane, float *sa) {
    // The recursion runs in log2 units (alpha2 = alpha * log2 e): v_exp_f32 / v_log_f32 are
    // base-2, so this drops four multiplies per state update; "-inf" is a large finite sentinel,
    // which removes the all-(-inf) special case (exp2(0) = 1, and the sentinel absorbs the rest).
    const float NEG = -1e30f, LOG2E = 1.44269504088896340736f;
    int S = 2 * L + 1;
    int tok[NS];
    bool skip_ok[NS];
    float a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        int s = lane * NS + k;
        tok[k] = QV_BLANK;
        skip_ok[k] = false;
        if (s < S && (s & 1)) {
            tok[k] = tgt[s >> 1];
            skip_ok[k] = s > 1 && tgt[s >> 1] != tgt[(s >> 1) - 1];
        }
        a[k] = NEG;
        if (s == 0) a[k] = lp[QV_BLANK] * LOG2E;
        if (s == 1) a[k] = lp[tok[k]] * LOG2E;
    }
    // the gathers lp[t][tok] do not depend on the recurrence: fetch TCH frames ahead so their
    // L2 latency overlaps the exp/log chain instead of serialising with it.  (Requesting the NEXT group before this
    // one's steps -- two register sets -- was measured: 70 -> 131 VGPRs, 7 -> 3 waves per SIMD, 144 -> 190 us.  The
    // kernel has ~200 leader waves per utterance and is bound by how many of them a SIMD interleaves, not by one
    // wave's latency.)
    constexpr int TCH = NS <= 2 ? 8 : (NS <= 6 ? 4 : 2);
    for (int t0 = 1; t0 < T; t0 += TCH) {
        float lpv[TCH][NS];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            int t = t0 + j < T ? t0 + j : T - 1;
            const float *row = lp + (size_t)t * QV_VOCAB;
#pragma unroll
            for (int k = 0; k < NS; ++k) lpv[j][k] = row[tok[k]] * LOG2E;
        }
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            if (t0 + j >= T) break;
            // previous lane's last two states
            float p1 = __shfl_up(a[NS - 1], 1), p2 = NS >= 2 ? __shfl_up(a[NS - 2], 1) : __shfl_up(a[NS - 1], 2);
            if (lane == 0) { p1 = NEG; p2 = NEG; }
            if (NS == 1 && lane == 1) p2 = NEG;
            float na[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                float la1 = a[k];
                float la2 = k >= 1 ? a[k - 1] : p1;
                float la3 = k >= 2 ? a[k - 2] : (k == 1 ? p1 : p2);
                if (NS == 1) la3 = p2;
                if (!skip_ok[k]) la3 = NEG;
                // log-sum-exp of three: the largest term is exp2(0) = 1 exactly, so only the other two need the
                // transcendental unit (the kernel is bound by v_exp_f32 / v_log_f32 issue: 4 -> 3 per state and frame)
                const float lamax = __builtin_fmaxf(la1, __builtin_fmaxf(la2, la3));
                const float lamin = __builtin_fminf(la1, __builtin_fminf(la2, la3));
                const float lamed = __builtin_fmaxf(__builtin_fminf(la1, la2), __builtin_fminf(__builtin_fmaxf(la1, la2), la3));
                // states beyond 2L never feed a lower state, so they are left unmasked
                na[k] = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(lamed - lamax) + __builtin_amdgcn_exp2f(lamin - lamax)) +
                        lamax + lpv[j][k];
            }
#pragma unroll
            for (int k = 0; k < NS; ++k) a[k] = na[k];
        }
    }
    // alpha_T of every state, for the caller's read-outs (its own target and the prefixes it leads)
#pragma unroll
    for (int k = 0; k < NS; ++k) sa[lane * NS + k] = a[k];
}

// Single-instruction three-operand forms (the compiler pads fmaxf / fminf chains with canonicalising v_max_f32 x, x
// because a gathered log-prob could be a signalling NaN; it never is here)
__device__ __forceinline__ float f_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float f_min3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float f_med3(float a, float b, float c) { float r; asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float f_max2(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float f_min2(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// Round 6: the same recursion with fewer instructions per state and frame -- same operands, same operation order, same
// bits as ctc_wave (tests/test_gpu_postlogits.py compares the two on every instantiation):
//  * with an even NS the parity of state lane*NS + k is the parity of k, a compile-time constant per register: even
//    states are blanks, whose third term (the skip transition) does not exist -- ctc_wave adds exp2(NEG - max) = +0 for
//    it -- so they take a two-term log-sum-exp (2 instead of 3 transcendental issues, 6 instead of ~14 VALU), and
//    their emission is the one value row[blank] per frame instead of a gather per state;
//  * max / min / median of three as v_max3 / v_min3 / v_med3 (one instruction each);
//  * states updated in place from the highest register down (a[k] needs the OLD a[k-1], a[k-2]): no copy pass.
// The kernel is bound by VALU + transcendental issue (sum over leaders of T x states, ~2.6 G state steps per batch of
// 64 gated 30 s clips), so this is where its time goes: 116 -> ~72 issue cycles per state and frame.
template <int NS>
__device__ void ctc_wave2(const float *__restrict__ lp, int T, const uint16_t *__restrict__ tgt, int L, int lane, float *sa) {
    const float NEG = -1e30f, LOG2E = 1.44269504088896340736f;
    constexpr bool PAR = (NS % 2) == 0;
    int S = 2 * L + 1;
    int tok[NS];
    bool skip_ok[NS];
    float a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        int s = lane * NS + k;
        tok[k] = QV_BLANK;
        skip_ok[k] = false;
        if (s < S && (s & 1)) {
            tok[k] = tgt[s >> 1];
            skip_ok[k] = s > 1 && tgt[s >> 1] != tgt[(s >> 1) - 1];
        }
        a[k] = NEG;
        if (s == 0) a[k] = lp[QV_BLANK] * LOG2E;
        if (s == 1) a[k] = lp[tok[k]] * LOG2E;
    }
    // (a parity-specialised lane gathers only its NS / 2 token states + the one blank value per frame: four frames ahead fit
    // the registers up to NS = 8, where the generic program stopped at NS = 6)
    constexpr int TCH = NS <= 2 ? 8 : (NS <= (PAR ? 8 : 6) ? 4 : 2);
    for (int t0 = 1; t0 < T; t0 += TCH) {
        float lpv[TCH][NS], lpb[TCH];
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            int t = t0 + j < T ? t0 + j : T - 1;
            const float *row = lp + (size_t)t * QV_VOCAB;
            if (PAR) lpb[j] = row[QV_BLANK] * LOG2E;
#pragma unroll
            for (int k = 0; k < NS; ++k)
                if (!PAR || (k & 1)) lpv[j][k] = row[tok[k]] * LOG2E;
        }
#pragma unroll
        for (int j = 0; j < TCH; ++j) {
            if (t0 + j >= T) break;
            float p1 = __shfl_up(a[NS - 1], 1), p2 = NS >= 2 ? __shfl_up(a[NS - 2], 1) : __shfl_up(a[NS - 1], 2);
            if (lane == 0) { p1 = NEG; p2 = NEG; }
            if (NS == 1 && lane == 1) p2 = NEG;
#pragma unroll
            for (int k = NS - 1; k >= 0; --k) {
                const float la1 = a[k];
                const float la2 = k >= 1 ? a[k - 1] : p1;
                if (PAR && !(k & 1)) {
                    const float hi2 = f_max2(la1, la2), lo2 = f_min2(la1, la2);
                    a[k] = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(lo2 - hi2)) + hi2 + lpb[j];
                } else {
                    float la3 = k >= 2 ? a[k - 2] : (k == 1 ? p1 : p2);
                    if (NS == 1) la3 = p2;
                    if (!skip_ok[k]) la3 = NEG;
                    const float lamax = f_max3(la1, la2, la3), lamin = f_min3(la1, la2, la3), lamed = f_med3(la1, la2, la3);
                    a[k] = __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(lamed - lamax) + __builtin_amdgcn_exp2f(lamin - lamax)) +
                           lamax + lpv[j][k];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) sa[lane * NS + k] = a[k];
}

// loss of the target made of the first P tokens, from the alpha_T row a recursion over at least P tokens left
// in `sa` (log2 units): -ln(alpha_T(2P) + alpha_T(2P - 1)), INFINITY when no alignment exists.
__device__ __forceinline__ float ctc_readout(const float *sa, int P) {
    const float LN2 = 0.693147180559945309417f;
    const float l1 = sa[2 * P], l2 = sa[2 * P - 1];
    const float m = fmaxf(l1, l2);
    const float ll2 = __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(l1 - m) + __builtin_amdgcn_exp2f(l2 - m)) + m;
    if (ll2 < -1e29f) return INFINITY;  // no alignment (the caller applies zero_infinity)
    return -ll2 * LN2;
}

// LONG = engine capacity above 30 s (more than 384 states per target): only then are the wide
// instantiations compiled into the kernel, keeping the common kernel's register footprint small
template <bool LONG, int VAR>
__device__ void ctc_dispatch(const float *lp, int T, const uint16_t *tgt, int L, int lane, float *sa) {
    int S = 2 * L + 1;
    if (VAR == 0) {     // the wave program of rounds 1-5 (QVERSE_CTC=0 / qv_debug_kernel_variant(4, 0)): cross-check only
        if (S <= 64) return ctc_wave<1>(lp, T, tgt, L, lane, sa);
        if (S <= 128) return ctc_wave<2>(lp, T, tgt, L, lane, sa);
        if (S <= 192) return ctc_wave<3>(lp, T, tgt, L, lane, sa);
        if (S <= 256) return ctc_wave<4>(lp, T, tgt, L, lane, sa);
        if (S <= 384 || !LONG) return ctc_wave<6>(lp, T, tgt, L, lane, sa);
        if (S <= 512) return ctc_wave<8>(lp, T, tgt, L, lane, sa);
        return ctc_wave<12>(lp, T, tgt, L, lane, sa);
    }
    if (S <= 64) return ctc_wave2<1>(lp, T, tgt, L, lane, sa);
    if (S <= 128) return ctc_wave2<2>(lp, T, tgt, L, lane, sa);
    if (S <= 192) return ctc_wave2<3>(lp, T, tgt, L, lane, sa);
    if (S <= 256) return ctc_wave2<4>(lp, T, tgt, L, lane, sa);
    if (S <= 384 || !LONG) return ctc_wave2<6>(lp, T, tgt, L, lane, sa);
    if (S <= 512) return ctc_wave2<8>(lp, T, tgt, L, lane, sa);
    return ctc_wave2<12>(lp, T, tgt, L, lane, sa);
}

// One wave per LEADER candidate (k_candidates' plan): one alpha recursion, then the loss of the leader and of
// every candidate whose ids are a prefix of its ids.
template <bool LONG, int VAR>
__global__ __launch_bounds__(256) void k_ctc(QvTables tab, QvWork wk, QvKnobs kn, const float *__restrict__ lp, int t_max) {
    __shared__ float sa_all[4][LONG ? 768 : 384];
    // grid = (utterance, block of four leader slots): the hardware dispatches workgroups x-fastest, and k_candidates sorted the
    // leaders by decreasing state count -- so EVERY utterance's longest recursions start first and the shortest ones fill the tail
    // (with the utterance on y, the last utterances' long leaders started when everything else was done)
    if ((int)blockIdx.x >= *wk.n_fail) return;
    int b = wk.fail_list[blockIdx.x];
    const QvUtt &u = wk.utt[b];
    if (!u.use_ctc) return;
    int lane = threadIdx.x & 63, wave = blockIdx.y * 4 + (threadIdx.x >> 6), nwave = gridDim.y * 4;
    float *sa = sa_all[threadIdx.x >> 6];
    int T = u.t_frames;
    const float *lpb = lp + (size_t)b * t_max * QV_VOCAB;
    const int16_t *lead = wk.cand_lead + (size_t)b * QV_CAND_CAP;
    for (int i = wave; i < u.n_lead; i += nwave) {
        const int c = lead[i];
        const int st = wk.cand_start[(size_t)b * QV_CAND_CAP + c], sp = wk.cand_span[(size_t)b * QV_CAND_CAP + c];
        const size_t k0 = (size_t)st * QV_MAX_SPAN;
        const int L = (int)(tab.tok_off[k0 + sp] - tab.tok_off[k0 + sp - 1]);
        ctc_dispatch<LONG, VAR>(lpb, T, tab.tok + tab.tok_off[k0 + sp - 1], L, lane, sa);
        // the leader itself (k == sp) and its members
        const int16_t *memb = wk.cand_memb + ((size_t)b * QV_CAND_CAP + c) * QV_MAX_SPAN;
        for (int k = 1; k <= sp; ++k) {
            const int m = k == sp ? c : (int)memb[k - 1];
            if (m < 0) continue;
            const int P = (int)(tab.tok_off[k0 + k] - tab.tok_off[k0 + k - 1]);
            float loss = ctc_readout(sa, P);
            if (isinf(loss)) loss = 0.f;  // zero_infinity=True
            float norm = __fdiv_rn(loss, (float)P);
            // -norm + TEXT_WEIGHT*text_score - SPAN_PENALTY*(span_len-1), in Python doubles
            double tw = __dmul_rn(kn.text_weight, wk.cand_score[(size_t)b * QV_CAND_CAP + m]);
            double fin = __dsub_rn(__dadd_rn(-(double)norm, tw), __dmul_rn(kn.span_penalty, (double)(k - 1)));
            if (lane == 0) {
                wk.cand_loss[(size_t)b * QV_CAND_CAP + m] = loss;
                wk.cand_final[(size_t)b * QV_CAND_CAP + m] = fin;
            }
        }
    }
}
