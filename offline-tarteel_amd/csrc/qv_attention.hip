// qv_attention.hip -- the rel-pos attention kernels of the FastConformer forward and their launcher: QK^T, the rel-pos
// term and PV on v_mfma_f32_32x32x16_f16 (V is produced already transposed by the QKV GEMM epilogue so that PV's A operand
// is K-contiguous).  Which kernel a batch gets: attention_plan (qv_launch_plan.h); what the kernels share: qv_att_wave.h.

#include "qv_layers.h"

#include "qv_att_wave.h"
#include "qv_launch_plan.h"

namespace {

// ------------------------------------------------------------------ attention ----------
// RelPositionMultiHeadAttention core for one (utterance, head): flash-style online softmax over
// 32-key tiles, one wave per 32-query tile, everything on v_mfma_f32_32x32x16_f16.
//   AC[i,j]  = (q_i + u) . k_j
//   BD[i,j]  = (q_i + v) . p_{T-1-i+j}          (rel_shift of the [T, 2T-1] product)
//   out      = softmax((AC + BD) / 8, keys < len) V
// All products are computed TRANSPOSED (keys / positions / head-dim on the MFMA row axis, queries
// on the column axis), so a lane owns ONE query: its 16 accumulator registers are 16 keys of that
// query, the softmax reductions are in-register plus one cross-half shuffle, the running max / sum
// are per-lane scalars, and exp(S^T) is already in the B-operand layout of the P.V product (the
// contraction index is permuted identically on the V side, which only changes which 8-byte pieces
// of V^T a lane loads).  The rel-pos term needs raw[c = 31 - i + j]: the two raw tiles go through
// a per-wave LDS slab (row = query, odd stride) and come back skewed.
// This kernel (variant 2) keeps its own tile body -- scaled units, explicit 31 - ii + jj columns, fragments straight from
// global memory: it is the independently written program the bit-for-bit tests hold the shared wave program against.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_attention(const half_t *__restrict__ qk, const half_t *__restrict__ vt,
                                                   const half_t *__restrict__ pos, int pos_ld, const float *__restrict__ bias_u,
                                                   const float *__restrict__ bias_v, const int32_t *__restrict__ len,
                                                   const int32_t *__restrict__ row_off, half_t *__restrict__ out, int t_max,
                                                   int t_pad) {
    __shared__ float slab[4][32 * ATT_LDS_LD];
    const int b = blockIdx.y, h = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int T = len[b];
    const size_t row0 = (size_t)row_off[b];   // activations are packed: utterance b owns rows [row0, row0 + T)
    const int l31 = lane & 31, hi = lane >> 5;
    const half_t *qb = qk + row0 * (2 * QV_D) + h * QV_DK;                           // q row stride 1024
    const half_t *kb = qb + QV_D;
    const half_t *vb = vt + ((size_t)b * QV_D + h * QV_DK) * t_pad;                  // [64][t_pad]
    const half_t *pb = pos + h * QV_DK;                                             // [2*t_max-1][pos_ld]
    const int n_qt = (T + 31) >> 5, n_kt = (T + 31) >> 5;
    float *sl = slab[wave];
    for (int qt = wave; qt < n_qt; qt += 4) {
        const int i0 = qt * 32;
        half_t *orow = out + (row0 + i0) * QV_D + h * QV_DK;
        half8 qu[4], qv[4];
        {
            int qi = i0 + l31;
            qi = qi < T ? qi : T - 1;   // never touch another utterance's rows
            half8 q8[4];
            att_query_load(qb, qi, hi, q8);
            att_query_bias(q8, bias_u, bias_v, h, hi, qu, qv);
        }
        f32x16 o0, o1;  // O^T: rows d (0..31 / 32..63), column = this lane's query
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
        float m_run = -1e30f, l_run = 0.f;
        // fragments of one key tile: K rows, the two position tiles, V^T pieces (in the key order of the P.V operand)
        struct TileKP { half8 kf[4], p0[4], p1[4]; };
        struct TileV { half4 a0[2], a1[2], c0[2], c1[2]; };
        auto fetch_kp = [&](int kt, TileKP &f) {
            const int j0 = kt * 32;
            int kj = j0 + l31;
            kj = kj < T ? kj : T - 1;
            // relative-position rows for this tile: rr0 + c, c in [0,64)
            const int rr0 = t_max - 1 - i0 - 31 + j0;
            int pr0 = rr0 + l31, pr1 = rr0 + 32 + l31;
            pr0 = pr0 < 0 ? 0 : (pr0 > 2 * t_max - 2 ? 2 * t_max - 2 : pr0);
            pr1 = pr1 < 0 ? 0 : (pr1 > 2 * t_max - 2 ? 2 * t_max - 2 : pr1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                int d = ks * 16 + hi * 8;
                f.kf[ks] = *(const half8 *)(kb + (size_t)kj * (2 * QV_D) + d);
                f.p0[ks] = *(const half8 *)(pb + (size_t)pr0 * pos_ld + d);
                f.p1[ks] = *(const half8 *)(pb + (size_t)pr1 * pos_ld + d);
            }
        };
        auto fetch_v = [&](int kt, TileV &f) {
            const int j0 = kt * 32;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                int jb = j0 + 16 * ks + 4 * hi;  // < t_pad
                f.a0[ks] = *(const half4 *)(vb + (size_t)l31 * t_pad + jb);
                f.a1[ks] = *(const half4 *)(vb + (size_t)l31 * t_pad + jb + 8);
                f.c0[ks] = *(const half4 *)(vb + (size_t)(32 + l31) * t_pad + jb);
                f.c1[ks] = *(const half4 *)(vb + (size_t)(32 + l31) * t_pad + jb + 8);
            }
        };
        auto tile = [&](int kt, const TileKP &cur, const TileV &cv) {
            const int j0 = kt * 32;
            f32x16 st, r0, r1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; r0[r] = 0.f; r1[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                st = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.kf[ks], qu[ks], st, 0, 0, 0);   // S^T[jj][ii]
                r0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.p0[ks], qv[ks], r0, 0, 0, 0);   // raw^T[c][ii], c < 32
                r1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.p1[ks], qv[ks], r1, 0, 0, 0);   // raw^T[32 + c][ii]
            }
            // skew through LDS: slab[ii][c] <- raw^T[c][ii]; BD^T[jj][ii] = slab[ii][31 - ii + jj]
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int c = att_row(r) + 4 * hi;
                sl[l31 * ATT_LDS_LD + c] = r0[r];
                sl[l31 * ATT_LDS_LD + 32 + c] = r1[r];
            }
            __builtin_amdgcn_wave_barrier();
            float p[16];
            float mx = -1e30f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int jj = att_row(r) + 4 * hi;
                float bd = sl[l31 * ATT_LDS_LD + 31 - l31 + jj];
                float sc = (st[r] + bd) * 0.125f;
                p[r] = (j0 + jj < T) ? sc : -1e30f;
                mx = fmaxf(mx, p[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float m_new = fmaxf(m_run, mx);
            float corr = __expf(m_run - m_new);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int jj = att_row(r) + 4 * hi;
                float e = (j0 + jj < T) ? __expf(p[r] - m_new) : 0.f;
                p[r] = e;
                sum += e;
            }
            sum += __shfl_xor(sum, 32);
            l_run = l_run * corr + sum;
            m_run = m_new;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= corr; o1[r] *= corr; }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) att_pv(o0, o1, att_p_frag(p, ks), cv.a0[ks], cv.a1[ks], cv.c0[ks], cv.c1[ks]);
        };
        for (int kt = 0; kt < n_kt; ++kt) {
            TileKP cur;
            TileV cv;
            fetch_kp(kt, cur);
            fetch_v(kt, cv);
            tile(kt, cur, cv);
        }
        if (i0 + l31 < T) att_store_out(o0, o1, 1.f / l_run, orow + (size_t)l31 * QV_D, hi);
    }
}

// Short utterances (T <= 128 encoder frames: every 10 s clip of the headline batch is 126).  The key-tiled kernel below
// walks the keys tile by tile with an online softmax, which for four key tiles is four times (stage -> barrier ->
// fragments -> MFMA -> skew through LDS -> softmax -> MFMA) in a row: 16 us of dependent chain for 0.5 us of MFMA.
// Here a block is one (utterance, head): its four waves (one query tile each) stage ALL of K, V^T and the 256
// relative-position rows the four query tiles can touch with coalesced direct-to-LDS loads (16 wave-loads per wave, one
// latency, one barrier; a first version that fetched the fragments straight from global memory -- 56 scattered loads per
// wave, every wave of the block fetching the same K and V -- ran 25 us, bound by the vector-memory pipeline), then each
// wave issues the K / position products of the WHOLE key range back to back (<= 16 + 20 MFMAs: the five position tiles
// of its 160-row window are each computed once, not once per key tile that touches them), skews tile after tile through
// its LDS slab (which takes the place of K and the position rows after a second barrier), takes ONE softmax over the
// complete row (no running maximum, no rescaling of the output accumulator) and ends with the <= 16 P.V products.
// 64 KB of LDS and < 256 registers: two blocks per CU, the headline batch (512 blocks) in one round.  Not the same
// summation as the key-tiled kernels (single-pass softmax), so not bit-identical to them; WHICH kernel an utterance gets
// depends on its own length only, never on the batch around it, so an utterance alone and in any batch has the same bits.
// (ATT_SHORT_T = 128: qv_limits.h)
#ifdef QV_ATT_STAMPS   // tools/att_bench.hip: shader-clock stamps of one block's waves at the phase boundaries
__device__ long long g_att_stamp[4][8];
#define ATT_STAMP(i) do { if (blockIdx.x == 3 && blockIdx.y == 17 && lane == 0) g_att_stamp[wave][i] = clock64(); } while (0)
#else
#define ATT_STAMP(i) do { } while (0)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_attention_short(
    const half_t *__restrict__ qk, const half_t *__restrict__ vt, const half_t *__restrict__ pos, int pos_ld,
    const float *__restrict__ bias_u, const float *__restrict__ bias_v, const int32_t *__restrict__ len,
    const int32_t *__restrict__ row_off, half_t *__restrict__ out, int t_max, int t_pad) {
    // [0, 16 K): K as 4 tiles [32 keys][64]; [16 K, 48 K): 256 position rows [64] (a ring that never wraps); [48 K, 64 K):
    // V^T as 4 tiles [64 d][32 keys] -- the layouts of qv_att_wave.h.
    // The four skew slabs (34,304 B) reuse [0, 48 K) once every wave has its K / position products.
    __shared__ __attribute__((aligned(16))) char smem[64 * 1024];
    half_t *sK = (half_t *)smem, *sP = (half_t *)(smem + 16 * 1024), *sV = (half_t *)(smem + 48 * 1024);
    // (round 5: handing XCD k the k-th eighth of the (utterance, head) pairs -- xcd_order, as in the LayerNorms -- was
    // measured: 16.46 -> 16.72 us; the kernel is not waiting for its K / V rows.  Kept head-major.)
    const int b = blockIdx.y, h = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int T = len[b];
    if (T > ATT_SHORT_T) return;                // whole block: a long utterance belongs to k_attention_ws
    ATT_STAMP(0);
    const size_t row0 = (size_t)row_off[b];
    const int l31 = lane & 31, hi = lane >> 5;
    const int i0 = wave * 32;
    const bool active = i0 < T;
    const half_t *qb = qk + row0 * (2 * QV_D) + h * QV_DK;
    const half_t *kb = qb + QV_D;
    const half_t *vb = vt + ((size_t)b * QV_D + h * QV_DK) * t_pad;
    const half_t *pb = pos + h * QV_DK;
    const int n_kt = (T + 31) >> 5;             // 1..4 key tiles = query tiles
    const int Rb = t_max - 128;                 // position row of window row 0
    // the query rows first: their latency is the longest chain in front of the first product (convert, add the biases)
    half8 q8[4];
    {
        int qi = i0 + l31;
        qi = qi < T ? qi : T - 1;
        att_query_load(qb, qi, hi, q8);
    }
    // ---- stage: wave w loads keys 8 w .. 8 w + 7 of every key tile, d rows 16 w .. of every V^T tile, its share of the
    // position rows [96 - 32 (n_kt - 1), 96 + 32 (n_kt + 1)) that the active query tiles touch
    for (int kt = 0; kt < n_kt; ++kt) att_stage_kv(kb, vb, t_pad, kt * 32, T, wave, lane, sK + kt * 2048, sV + kt * 2048);
    att_stage_pos<256>(pb, pos_ld, Rb, t_max, 32 * (4 - n_kt), 8 * n_kt, wave, lane, sP);
    half8 qu[4], qv[4];
    att_query_bias(q8, bias_u, bias_v, h, hi, qu, qv);
    ATT_STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    ATT_STAMP(2);
    // S^T[kt][jj][ii] for every key tile, raw^T[pt][c][ii] for position tiles pt = 0 .. n_kt (window rows 96 - i0 + 32 pt + c)
    f32x16 st[4], raw[5];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[kt][r] = 0.f;
        if (active && kt < n_kt) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                half8 kf = *(const half8 *)(sK + kt * 2048 + l31 * 64 + att_kcol(l31, hi, ks));
                st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qu[ks], st[kt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int pt = 0; pt < 5; ++pt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) raw[pt][r] = 0.f;
        if (active && pt <= n_kt) {
            const int wr = 96 - i0 + 32 * pt + l31;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                half8 pf = *(const half8 *)(sP + wr * 64 + att_kcol(wr, hi, ks));
                raw[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, qv[ks], raw[pt], 0, 0, 0);
            }
        }
    }
    __syncthreads();                            // K and the position rows are dead: the slabs take their place
    if (!active) return;
    ATT_STAMP(3);
    float *sl = (float *)smem + wave * (32 * ATT_LDS_LD);
    // skew tile by tile: BD^T of key tile kt is slab[ii][31 - ii + jj] over the 64 columns (raw^T tile kt | tile kt + 1).
    // Every position tile is written ONCE: tile pt lives in slab columns 32 (pt & 1) .., so key tile kt finds tile kt in
    // one half and only tile kt + 1 has to replace tile kt - 1 in the other; the read column wraps modulo 64.
    // st[kt] becomes the masked, scaled score
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sl[l31 * ATT_LDS_LD + att_row(r) + 4 * hi] = raw[0][r];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt < n_kt) {
            __builtin_amdgcn_wave_barrier();    // the reads of key tile kt - 1 are issued before tile kt + 1 lands on tile kt - 1
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sl[l31 * ATT_LDS_LD + 32 * ((kt + 1) & 1) + att_row(r) + 4 * hi] = raw[kt + 1][r];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int jj = att_row(r) + 4 * hi;
                float bd = sl[l31 * ATT_LDS_LD + ((32 * (kt & 1) + 31 - l31 + jj) & 63)];
                float sc = (st[kt][r] + bd) * 0.125f;
                sc = (kt * 32 + jj < T) ? sc : -1e30f;
                st[kt][r] = sc;
                mx = fmaxf(mx, sc);
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    ATT_STAMP(4);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt < n_kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int jj = att_row(r) + 4 * hi;
                float e = (kt * 32 + jj < T) ? __expf(st[kt][r] - mx) : 0.f;
                st[kt][r] = e;
                sum += e;
            }
        }
    }
    sum += __shfl_xor(sum, 32);
    ATT_STAMP(5);
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt < n_kt) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const half8 pbf = att_p_frag(st[kt], ks);
                half4 a0, a1, c0, c1;
                att_v_pieces(sV + kt * 2048, att_vd(l31, hi), att_vd(32 + l31, hi), att_vswz(l31), ks, a0, a1, c0, c1);
                att_pv(o0, o1, pbf, a0, a1, c0, c1);
            }
        }
    }
    if (i0 + l31 < T) att_store_out(o0, o1, 1.f / sum, out + (row0 + i0 + l31) * QV_D + h * QV_DK, hi);
    ATT_STAMP(6);
}

// Wave-specialised version of the same computation (same arithmetic, same order).  k_attention's
// duration is one wave's serial chain -- per key tile two exposed global-load latencies (K and
// position fragments, then V) in front of 16 MFMAs -- and it keeps a wave busy with one query tile
// after the other for long utterances.  Here a block is one (head, utterance, group of 4 query
// tiles): waves 0..3 are consumers (one query tile each; fragments come from LDS), waves 4..7 are
// loaders that stage, TWO key tiles ahead (3 buffers), the K tile (32 keys x 64), the V^T tile
// (64 x 32 keys) and the 32 NEW relative-position rows of the tile: the position rows the four query
// tiles need form a sliding window of 160 rows that advances by 32 per key tile, kept in a 256-row
// ring (window of tile kt + the 64 rows prefetched for kt + 1 and kt + 2 never overlap in it).
// HPB heads share a block (4 consumer waves each; the 4 loader waves stage for all of them): with HPB = 2 every SIMD runs
// two consumer waves whose serial chains (MFMA -> skew through LDS -> softmax -> MFMA) overlap, and B = 64 x 10 s is one
// round of 256 blocks instead of two rounds of 512.  LDS then only holds NST = 2 K/V stages (tile kt + 1 is requested
// when tile kt's barrier frees the other buffer) and a 192-row position ring (160-row window + the 32 rows of the next
// tile).  The arithmetic of a (head, query tile) is the same wave program in both shapes (AttWave, qv_att_wave.h):
// outputs are bit-identical.
template <int HPB, int NST, int RING>
__global__ __launch_bounds__(256 * HPB + 256) void k_attention_ws(const half_t *__restrict__ qk, const half_t *__restrict__ vt,
                                                                  const half_t *__restrict__ pos, int pos_ld,
                                                                  const float *__restrict__ bias_u, const float *__restrict__ bias_v,
                                                                  const int32_t *__restrict__ len, const int32_t *__restrict__ row_off,
                                                                  half_t *__restrict__ out, int t_max, int t_pad, int t_short) {
    static_assert(RING % 8 == 0 && RING >= 160 + 32 * (NST - 1), "position ring: window + prefetched rows");
    __shared__ __attribute__((aligned(16))) half_t sK[HPB][NST][32 * 64];
    __shared__ __attribute__((aligned(16))) half_t sV[HPB][NST][64 * 32];
    __shared__ __attribute__((aligned(16))) half_t sP[HPB][RING * 64];       // ring of position rows
    __shared__ float slab[4 * HPB][32 * ATT_LDS_LD];
    const int b = blockIdx.z, qg = blockIdx.y, hg = blockIdx.x;
    const int T = len[b];
    if (qg * 128 >= T || T <= t_short) return;       // whole block: no query of this group exists / k_attention_short's utterance
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool loader = wave >= 4 * HPB;
    const int w4 = wave & 3, l31 = lane & 31, hi = lane >> 5;
    const size_t row0 = (size_t)row_off[b];
    const int n_kt = (T + 31) >> 5;
    const int Rb = t_max - 128 * qg - 128;           // first position row of key tile 0's window

    if (loader) {
        // per head: one K, one V and one position load per loader wave and key tile (1 KB each)
        auto stage = [&](int kt) {
#pragma unroll
            for (int hh = 0; hh < HPB; ++hh) {
                const int h = hg * HPB + hh;
                att_stage_kv(qk + row0 * (2 * QV_D) + QV_D + h * QV_DK, vt + ((size_t)b * QV_D + h * QV_DK) * t_pad, t_pad, kt * 32, T,
                             w4, lane, sK[hh][kt % NST], sV[hh][kt % NST]);
            }
        };
        auto pos_rows = [&](int first, int n8) {   // n8 chunks of 8 rows starting at window row `first`, this wave's share
            att_stage_pos<RING>(pos + hg * HPB * QV_DK, pos_ld, Rb, t_max, first, n8, w4, lane, sP[0], HPB);
        };
        // per wave: unit(0) = HPB x (5 position chunks + K + V), unit(kt >= 1) = HPB x (K + V + 1 position chunk)
        pos_rows(0, 20);        // rows 0 .. 159: the window of tile 0
        stage(0);
        if (NST == 3 && n_kt > 1) {
            stage(1);
            pos_rows(32 + 128, 4);
        }
        for (int kt = 0; kt < n_kt; ++kt) {
            WS_STAMP(kt, 0);
            // unit(kt) has landed once only the units requested after it may still be in flight
            if (NST == 3 && kt + 1 < n_kt) {
                if (HPB == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            WS_STAMP(kt, 1);
            __builtin_amdgcn_s_barrier();           // tile kt visible; the buffers of tile kt - 1 are free
            WS_STAMP(kt, 2);
            if (kt + NST - 1 < n_kt) {
                stage(kt + NST - 1);
                pos_rows(32 * (kt + NST - 1) + 128, 4);   // the 32 new rows of that tile
            }
            WS_STAMP(kt, 3);
        }
        return;
    }

    // ---------------------------------------------------------------- consumers ----------
    const int hh = wave >> 2, h = hg * HPB + hh;
    const int i0 = qg * 128 + w4 * 32;
    const bool active = i0 < T;
    AttWave<RING> w;
    w.init(qk + row0 * (2 * QV_D) + h * QV_DK, bias_u, bias_v, h, i0, T, l31, hi, w4, slab[wave]);
    for (int kt = 0; kt < n_kt; ++kt) {
        WS_STAMP(kt, 0);
        __builtin_amdgcn_s_barrier();
        WS_STAMP(kt, 1);
        if (!active) continue;
        w.template step<true>(kt, n_kt, sK[hh][0], sV[hh][0], sP[hh], [](int t) { return t % NST; });
    }
    if (active && i0 + l31 < T) w.store(out + (row0 + i0 + l31) * QV_D + h * QV_DK);
}

// Round 6, variant 4: the key-tiled computation WITHOUT loader waves and with TWO independent blocks per CU.
// k_attention_ws<2, 2, 192> is bound by the instruction issue of the two consumer waves of a SIMD, and those two run in lock
// step: both heads of a block leave the same barrier, so both are in their MFMA phase, then both in their softmax phase
// (stamps: tools/att_bench).  Here a block is ONE (head, 128-query group, utterance) with four waves that stage their own
// tiles -- each wave issues its quarter of the K, V^T and position loads of key tile kt + 1 (three 1 KB direct-to-LDS loads)
// right after the barrier that released tile kt -- in 74 KB of LDS and, without loader waves, 256 threads: two blocks per
// CU, 256 registers per wave.  The two consumer waves of a SIMD then belong to DIFFERENT blocks, whose barriers are
// independent: one wave's matrix products run under the other's softmax.  Same wave program per (head, query tile) as the
// other key-tiled shapes (AttWave) => the same bits (tests/test_gpu_forward.py compares variants 0, 1, 2 and 4).
template <int RING>
__global__ __launch_bounds__(256, 2) void k_attention_x(const half_t *__restrict__ qk, const half_t *__restrict__ vt,
                                                         const half_t *__restrict__ pos, int pos_ld,
                                                         const float *__restrict__ bias_u, const float *__restrict__ bias_v,
                                                         const int32_t *__restrict__ len, const int32_t *__restrict__ row_off,
                                                         half_t *__restrict__ out, int t_max, int t_pad, int t_short) {
    static_assert(RING % 32 == 0 && RING >= 160 + 32, "position ring: window + the rows of the next tile");
    __shared__ __attribute__((aligned(16))) half_t sK[2][32 * 64];
    __shared__ __attribute__((aligned(16))) half_t sV[2][64 * 32];
    __shared__ __attribute__((aligned(16))) half_t sP[RING * 64];       // ring of position rows
    __shared__ float slab[4][32 * ATT_LDS_LD];
    const int b = blockIdx.z, qg = blockIdx.y, h = blockIdx.x;
    const int T = len[b];
    if (qg * 128 >= T || T <= t_short) return;
    const int w4 = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const size_t row0 = (size_t)row_off[b];
    const int n_kt = (T + 31) >> 5;
    const int Rb = t_max - 128 * qg - 128;           // first position row of key tile 0's window
    const half_t *kb = qk + row0 * (2 * QV_D) + QV_D + h * QV_DK;
    const half_t *vb = vt + ((size_t)b * QV_D + h * QV_DK) * t_pad;
    const half_t *pb = pos + h * QV_DK;
    // this wave's quarter of key tile kt, and its share of n8 chunks of 8 position rows starting at window row `first`
    auto stage = [&](int kt) { att_stage_kv(kb, vb, t_pad, kt * 32, T, w4, lane, sK[kt & 1], sV[kt & 1]); };
    auto pos_rows = [&](int first, int n8) { att_stage_pos<RING>(pb, pos_ld, Rb, t_max, first, n8, w4, lane, sP); };
    pos_rows(0, 20);                                  // rows 0 .. 159: the window of tile 0
    stage(0);

    const int i0 = qg * 128 + w4 * 32;
    const bool active = i0 < T;
    AttWave<RING> w;
    w.init(qk + row0 * (2 * QV_D) + h * QV_DK, bias_u, bias_v, h, i0, T, l31, hi, w4, slab[w4]);
    for (int kt = 0; kt < n_kt; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's quarter of tile kt (and of its position rows) has landed ...
        __builtin_amdgcn_s_barrier();                        // ... and everybody's; everybody has left tile kt - 1's buffers
        if (kt + 1 < n_kt) {
            stage(kt + 1);
            pos_rows(32 * (kt + 1) + 128, 4);               // the 32 new rows of that tile
        }
        if (!active) continue;
        w.template step<false>(kt, n_kt, sK[0], sV[0], sP, [](int t) { return t & 1; });
    }
    if (active && i0 + l31 < T) w.store(out + (row0 + i0 + l31) * QV_D + h * QV_DK);
}

}  // namespace

// which kernels a batch gets: attention_plan (qv_launch_plan.h).  The caller passes the snapshot it took ONCE (a forward:
// qv_model.hip), so a test that flips the process-wide switch while batches of other contexts are in flight cannot change
// kernels between the layers of one forward
void launch_attention(const half_t *qk, const half_t *vt, const half_t *pos, int pos_ld, const float *bu, const float *bv,
                      const int32_t *len, const int32_t *row_off, half_t *out, int t_max, int t_min, int t_pad, int batch,
                      hipStream_t s, const QvSwitches &sw) {
    const AttentionPlan p = attention_plan(sw[QV_SW_ATT], t_min, t_max);
    if (p.run_short)
        hipLaunchKernelGGL(k_attention_short, dim3(QV_H, batch), dim3(256), 0, s, qk, vt, pos, pos_ld, bu, bv, len, row_off,
                           out, t_max, t_pad);
    switch (p.rest) {
    case ATT_OLD:
        hipLaunchKernelGGL(k_attention, dim3(QV_H, batch), dim3(256), 0, s, qk, vt, pos, pos_ld, bu, bv, len, row_off, out, t_max,
                           t_pad);
        break;
    case ATT_X_192:
        hipLaunchKernelGGL((k_attention_x<192>), dim3(QV_H, (t_max + 127) / 128, batch), dim3(256), 0, s, qk, vt, pos,
                           pos_ld, bu, bv, len, row_off, out, t_max, t_pad, p.t_short);
        break;
    case ATT_WS_1_3_256:
        hipLaunchKernelGGL((k_attention_ws<1, 3, 256>), dim3(QV_H, (t_max + 127) / 128, batch), dim3(512), 0, s, qk, vt, pos,
                           pos_ld, bu, bv, len, row_off, out, t_max, t_pad, p.t_short);
        break;
    case ATT_WS_2_2_192:
        hipLaunchKernelGGL((k_attention_ws<2, 2, 192>), dim3(QV_H / 2, (t_max + 127) / 128, batch), dim3(768), 0, s, qk, vt, pos,
                           pos_ld, bu, bv, len, row_off, out, t_max, t_pad, p.t_short);
        break;
    default: break;   // ATT_NONE: every utterance was the short kernel's
    }
}
