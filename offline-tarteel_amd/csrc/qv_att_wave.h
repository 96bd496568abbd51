// qv_att_wave.h -- what the attention kernels (qv_attention.hip, the only file that includes this) have in common, one
// definition each: the accumulator row map, the LDS layouts of a K tile, a V^T tile and the position rows with their write
// side (staging) next to their read side (fragment offsets), the query fragments, the P.V step, the output store, and the
// key-tiled wave program of k_attention_ws / k_attention_x.  Device only, no state outside AttWave; no floating-point
// operation here is reordered against the kernels that used to spell these out, so the kernels that share a helper keep
// their bits.
#pragma once

#include "qv_kernels.h"

#define ATT_LDS_LD 67  // floats per query row of the skew slab (odd: conflict-free skewed reads)

#ifdef QV_ATT_STAMPS   // tools/att_bench.hip: per key tile, clock stamps of every wave of ONE block of the key-tiled kernel
namespace {
__device__ long long g_ws_stamp[12][16][6];
}
#define WS_STAMP(kt, i) do { if (blockIdx.x == 1 && blockIdx.y == 1 && blockIdx.z == 17 && lane == 0 && (kt) < 16) g_ws_stamp[wave][kt][i] = clock64(); } while (0)
#else
#define WS_STAMP(kt, i) do { } while (0)
#endif

static __device__ __forceinline__ void att_glds16(const void *g, void *l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)l,
                                     16, 0, 0);
}

// row of register r in the 32 x 32 MFMA accumulator of a lane (+ 4 * hi for the upper half-wave)
static __device__ __forceinline__ constexpr int att_row(int r) { return (r & 3) + 8 * (r >> 2); }

// ---------------------------------------------------------------- LDS layouts: write side, read side ----------
// K tile [32 keys][64 d] and position rows [row][64 d]: the eight 16-B chunks of a row are swizzled by (row >> 1) & 7.
// V^T tile [64 d][32 keys]: the four 16-B chunks of a row by (d >> 2) & 3.
static __device__ __forceinline__ int att_kswz(int row) { return (row >> 1) & 7; }
static __device__ __forceinline__ int att_vswz(int d) { return (d >> 2) & 3; }

// write: wave w4's quarter of key tile j0 .. j0 + 31 (8 keys x 128 B of K, 16 d rows x 64 B of V^T; keys < t_pad), one
// direct-to-LDS load each.  Keys past the utterance read its last row: never another utterance's.
static __device__ __forceinline__ void att_stage_kv(const half_t *kb, const half_t *vb, int t_pad, int j0, int T, int w4, int lane,
                                                    half_t *sKt, half_t *sVt) {
    {
        int r = w4 * 8 + (lane >> 3), c = (lane & 7) ^ att_kswz(r);
        int kj = j0 + r;
        kj = kj < T ? kj : T - 1;
        att_glds16(kb + (size_t)kj * (2 * QV_D) + c * 8, sKt + w4 * 512);
    }
    {
        int r = w4 * 16 + (lane >> 2), c = (lane & 3) ^ att_vswz(r);
        att_glds16(vb + (size_t)r * t_pad + j0 + c * 8, sVt + w4 * 512);
    }
}
// write: wave w4's share of n8 chunks of 8 window rows starting at window row `first` (position row Rb + window row, clamped
// to the table's [0, 2 t_max - 2]) into a ring of RING rows, for `heads` heads (QV_DK apart in pb, a ring apart in sP)
template <int RING>
static __device__ __forceinline__ void att_stage_pos(const half_t *pb, int pos_ld, int Rb, int t_max, int first, int n8, int w4,
                                                     int lane, half_t *sP, int heads = 1) {
    for (int q = w4; q < n8; q += 4) {
        int wr = first + q * 8 + (lane >> 3);                 // row relative to Rb
        int ring = wr % RING;
        int c = (lane & 7) ^ att_kswz(ring);
        int rr = Rb + wr;
        rr = rr < 0 ? 0 : (rr > 2 * t_max - 2 ? 2 * t_max - 2 : rr);
#pragma unroll
        for (int hh = 0; hh < heads; ++hh)
            att_glds16(pb + hh * QV_DK + (size_t)rr * pos_ld + c * 8, sP + hh * (RING * 64) + (size_t)((first + q * 8) % RING) * 64);
    }
}
// read: A fragment (row, d = 16 ks + 8 hi ..) of a K tile or of the position rows is chunk 2 ks + hi of the row: row * 64 +
// att_kcol halves.  The K-step only flips bits 4-5 of that offset, so the wave program keeps ONE lane constant (K-step 0)
// and XORs: att_kf(att_kf0(row, hi), ks) == row * 64 + att_kcol(row, hi, ks)
static __device__ __forceinline__ int att_kcol(int row, int hi, int ks) { return ((ks * 2 + hi) ^ att_kswz(row)) << 3; }
static __device__ __forceinline__ int att_kf0(int row, int hi) { return row * 64 + att_kcol(row, hi, 0); }
static __device__ __forceinline__ int att_kf(int kf0, int ks) { return kf0 ^ (ks << 4); }
// read: the V^T pieces of P.V step ks for rows d = l31 (vda) and 32 + l31 (vdc), which share (d >> 2) & 3 (vsw): keys
// 16 ks + 4 hi + {0..3} and + 8 -> 16-B chunks 2 ks and 2 ks + 1, 8-byte half `hi`
static __device__ __forceinline__ int att_vd(int d, int hi) { return d * 32 + 4 * hi; }
static __device__ __forceinline__ void att_v_pieces(const half_t *sVt, int vda, int vdc, int vsw, int ks, half4 &a0, half4 &a1,
                                                    half4 &c0, half4 &c1) {
    a0 = *(const half4 *)(sVt + vda + (((2 * ks) ^ vsw) << 3));
    a1 = *(const half4 *)(sVt + vda + (((2 * ks + 1) ^ vsw) << 3));
    c0 = *(const half4 *)(sVt + vdc + (((2 * ks) ^ vsw) << 3));
    c1 = *(const half4 *)(sVt + vdc + (((2 * ks + 1) ^ vsw) << 3));
}

// ---------------------------------------------------------------- query fragments, P.V, output ----------
// B fragments (queries on the column axis) of query row qi (clamped by the caller), d = ks * 16 + hi * 8 ..: the load, then
// (q + u) and (q + v) in f32, rounded to f16.  Two calls: k_attention_short puts its staging loads between them.
static __device__ __forceinline__ void att_query_load(const half_t *qb, int qi, int hi, half8 q8[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) q8[ks] = *(const half8 *)(qb + (size_t)qi * (2 * QV_D) + ks * 16 + hi * 8);
}
static __device__ __forceinline__ void att_query_bias(const half8 q8[4], const float *bias_u, const float *bias_v, int h, int hi,
                                                      half8 qu[4], half8 qv[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        int d = ks * 16 + hi * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float qf = (float)q8[ks][e];
            qu[ks][e] = (half_t)(qf + bias_u[h * QV_DK + d + e]);
            qv[ks][e] = (half_t)(qf + bias_v[h * QV_DK + d + e]);
        }
    }
}
// P.V step ks: B operand (att_p_frag) = exp(S^T) registers 8 ks .. 8 ks + 7 (keys 16 ks + 4 hi + {0..3, 8..11}); A operand =
// V^T rows d (a: 0..31, c: 32..63) with the same key order, each assembled from two 8-byte pieces
template <typename P>
static __device__ __forceinline__ half8 att_p_frag(const P &p, int ks) {
    half8 pbf;
#pragma unroll
    for (int e = 0; e < 8; ++e) pbf[e] = (half_t)p[8 * ks + e];
    return pbf;
}
static __device__ __forceinline__ void att_pv(f32x16 &o0, f32x16 &o1, half8 pbf, half4 a0, half4 a1, half4 c0, half4 c1) {
    half8 va = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    half8 vc = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
    o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pbf, o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vc, pbf, o1, 0, 0, 0);
}
// O^T column of one query (o: its output row at the head's offset): d = att_row(r) + 4 * hi (+ 32)
static __device__ __forceinline__ void att_store_out(const f32x16 &o0, const f32x16 &o1, float inv, half_t *o, int hi) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int d = 8 * q + 4 * hi;
        half4 h0, h1;
#pragma unroll
        for (int e = 0; e < 4; ++e) { h0[e] = (half_t)(o0[4 * q + e] * inv); h1[e] = (half_t)(o1[4 * q + e] * inv); }
        *(half4 *)(o + d) = h0;
        *(half4 *)(o + 32 + d) = h1;
    }
}

// ---------------------------------------------------------------- the key-tiled wave program ----------
// One consumer wave = one (head, 32-query tile) walking the key tiles its kernel staged: k_attention_ws (REMAT = true) and
// k_attention_x (REMAT = false) run this one program, so their outputs are bit-identical.  w4 = the wave's query tile in its
// group of four; the position rows of the group sit in a ring of RING rows (att_stage_pos).
// Round 6.  The loop is bound by the instructions the two consumer waves of a SIMD issue per key tile (stamps in
// tools/att_bench: 4.4 k cycles per tile, the loaders land a tile ahead and wait), so the same arithmetic is issued
// with fewer of them -- the output bits do not change (tests compare variants 0 .. 2):
//  * scores stay in RAW units (8 x the scaled score) up to the exponential: exp((p - m) / 8) = exp2((p - m) * (log2 e / 8)),
//    and scaling by a power of two commutes with every rounding on the way -- 16 multiplies per tile gone;
//  * the key mask (j0 + jj < T) only exists in an utterance's LAST key tile: the other tiles run an unmasked copy of
//    the body (16 compares + 32 selects gone);
//  * the skew slab keeps alternating halves (tile kt sits where tile kt - 1 wrote it as ITS second tile), but the column
//    of a value is no longer computed with a wrap: an even key tile reads lane constant + immediate (31 - ii + jj <= 62
//    never wraps), an odd one reads the same column XOR 32, i.e. one of two lane-constant bases chosen by a compare of two
//    constants per value -- ~5 integer instructions per value read become 0 / 2;
//  * fragment addresses: lane constants computed once, XORed with the K-step.
template <int RING>
struct AttWave {
    static constexpr float NEG = -1e30f * 8.0f, L2E8 = 0x1.715476p+0f * 0.125f;   // (__expf(x) is v_exp_f32(x * 0x1.715476p+0))
    half8 qu[4], qv[4];
    f32x16 o0, o1;          // O^T: rows d (0..31 / 32..63), column = this lane's query
    float m_run, l_run;
    int T, hi, w4, kf0, vda, vdc, vsw, ring1;
    float *slw;             // slab stores: + 32 * tile + att_row(r)
    const float *slr;       // slab loads: + att_row(r), never past column 62
    unsigned hiw;

    // qb: the head's query rows of the utterance; i0: first query of the wave's tile; sl: the wave's skew slab
    __device__ __forceinline__ void init(const half_t *qb, const float *bias_u, const float *bias_v, int h, int i0, int T_,
                                         int l31, int hi_, int w4_, float *sl) {
        T = T_; hi = hi_; w4 = w4_;
        half8 q8[4];
        int qi = i0 + l31;
        qi = qi < T ? qi : T - 1;   // never touch another utterance's rows
        att_query_load(qb, qi, hi, q8);
        att_query_bias(q8, bias_u, bias_v, h, hi, qu, qv);
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
        m_run = NEG; l_run = 0.f;
        kf0 = att_kf0(l31, hi);
        slw = sl + l31 * ATT_LDS_LD + 4 * hi;
        slr = sl + l31 * ATT_LDS_LD + (31 - l31 + 4 * hi);
        // odd tiles: slab column = window column ^ 32, i.e. + 32 where the window column 31 - ii + jj is below 32 and - 32 elsewhere;
        // bit r of `hiw` says "elsewhere" for register r, so the address is one shift-add away from a lane constant
        hiw = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) hiw |= (unsigned)(att_row(r) >= 1 + l31 - 4 * hi) << r;
        vda = att_vd(l31, hi); vdc = att_vd(32 + l31, hi); vsw = att_vswz(l31);
        ring1 = (128 - 32 * w4) % RING;                          // position tile kt + 1 of this wave starts at ring row 32 kt + 128 - 32 w4
    }

    // key tile kt from the kernel's K / V^T stage buffers (sK0 / sV0: stage 0 of the head, 2048 halves a stage; stage_of(kt):
    // the stage tile kt sits in -- chosen inside the specialised body, after the (last, odd) dispatch: chosen in front of it,
    // the pointers stay live across the four copies and cost k_attention_x eight registers) and the head's position ring.
    // ODD: kt & 1 (never kt == 0)
    template <bool MASKED, bool ODD, bool REMAT, typename Stage>
    __device__ __forceinline__ void tile(int kt, const half_t *sK0, const half_t *sV0, const half_t *sPh, Stage stage_of) {
#ifdef QV_ATT_STAMPS
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#endif
        const int j0 = kt * 32;
        // (the per-K-step fragment offsets are re-derived from three lane constants in every tile -- one XOR / shift each: hoisted
        // out of the loop they are 14 more live registers, and the two-heads-per-block shape has 168 per wave)
        int kfl = kf0, val = vda, vcl = vdc;
        if (REMAT) asm volatile("" : "+v"(kfl), "+v"(val), "+v"(vcl));
        const half_t *sKb = sK0 + stage_of(kt) * 2048, *sVb = sV0 + stage_of(kt) * 2048;
        // position tile pt = rows 32 pt .. of the wave's window: key tile kt needs tiles kt and kt + 1, and tile kt is what
        // key tile kt - 1 computed as ITS second tile -- same operands, same products, so it is carried over instead of
        // being computed twice
        f32x16 st, r1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = 0.f; r1[r] = 0.f; }
        if (!ODD && kt == 0) {
            const int ring0 = (96 - 32 * w4) % RING;
            f32x16 r0;
#pragma unroll
            for (int r = 0; r < 16; ++r) r0[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                half8 p0 = *(const half8 *)(sPh + ring0 * 64 + att_kf(kfl, ks));
                r0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(p0, qv[ks], r0, 0, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) slw[att_row(r)] = r0[r];
        }
        const half_t *sP1 = sPh + ring1 * 64;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8 kf = *(const half8 *)(sKb + att_kf(kfl, ks));
            half8 p1 = *(const half8 *)(sP1 + att_kf(kfl, ks));
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qu[ks], st, 0, 0, 0);   // S^T[jj][ii]
            r1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, qv[ks], r1, 0, 0, 0);   // raw^T[32 + c][ii]
        }
        ring1 += 32;
        if (ring1 >= RING) ring1 -= RING;
        // skew: BD^T[jj][ii] = window[ii][31 - ii + jj], window = [tile kt | tile kt + 1]; tile pt lives in slab columns
        // 32 (pt & 1) .., so tile kt is already there and tile kt + 1 replaces tile kt - 1
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) slw[(ODD ? 0 : 32) + att_row(r)] = r1[r];
        __builtin_amdgcn_wave_barrier();
        WS_STAMP(kt, 2);
        float p[16];
        float mx = NEG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jj = att_row(r) + 4 * hi;
            const int e = att_row(r);
            // even tile: window column = slab column; odd tile: slab column = window column ^ 32
            const float bd = !ODD ? slr[e] : *(const float *)((const char *)(slr + 32 + e) - (((hiw >> r) & 1u) << 8));
            const float sc = st[r] + bd;
            p[r] = (!MASKED || j0 + jj < T) ? sc : NEG;
            mx = fmaxf(mx, p[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float corr = __builtin_amdgcn_exp2f((m_run - m_new) * L2E8);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jj = att_row(r) + 4 * hi;
            const float e = (!MASKED || j0 + jj < T) ? __builtin_amdgcn_exp2f((p[r] - m_new) * L2E8) : 0.f;
            p[r] = e;
            sum += e;
        }
        sum += __shfl_xor(sum, 32);
        l_run = l_run * corr + sum;
        m_run = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= corr; o1[r] *= corr; }
        WS_STAMP(kt, 3);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const half8 pbf = att_p_frag(p, ks);
            half4 a0, a1, c0, c1;
            att_v_pieces(sVb, val, vcl, vsw, ks, a0, a1, c0, c1);
            att_pv(o0, o1, pbf, a0, a1, c0, c1);
        }
        WS_STAMP(kt, 4);
    }

    // key tile kt of n_kt: the mask only in the last tile, the slab half by the tile's parity
    template <bool REMAT, typename Stage>
    __device__ __forceinline__ void step(int kt, int n_kt, const half_t *sK0, const half_t *sV0, const half_t *sPh, Stage stage_of) {
        if (kt + 1 < n_kt) { if (kt & 1) tile<false, true, REMAT>(kt, sK0, sV0, sPh, stage_of); else tile<false, false, REMAT>(kt, sK0, sV0, sPh, stage_of); }
        else { if (kt & 1) tile<true, true, REMAT>(kt, sK0, sV0, sPh, stage_of); else tile<true, false, REMAT>(kt, sK0, sV0, sPh, stage_of); }
    }

    // o: the output row of this lane's query at the head's offset
    __device__ __forceinline__ void store(half_t *o) const { att_store_out(o0, o1, 1.f / l_run, o, hi); }
};
