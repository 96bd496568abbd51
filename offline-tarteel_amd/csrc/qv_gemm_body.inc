// The body of k_gemm / k_gemm_pk (qv_gemm.hip includes this file once per kernel symbol: the two differ only in the target
// features they are compiled with).  Template parameters EPI, BN, WQ, NST, LD and the argument `GemmArgs g` are in scope.
// The epilogue's values come from qv_gemm_epilogue.h (shared with k_gemm256); the block-wide LDS staging is this kernel's own.
#define QV_TRACE(slot) QV_TRACE_AT((wave & 3) == 0, ((QV_BLOCK * 8 + wave) * 64 + kt_) * 4 + (slot))
    using namespace qv_epi;
    constexpr bool W4 = WQ == 4, W8 = WQ == 8;
    // A8W8 (QV_PREC_ORT_MIXED): both operands are bytes and K counts byte PAIRS, so loaders, LDS image and fragment
    // reads are the f16 kernel's unchanged -- a 16-byte fragment chunk is 16 k values for v_mfma_i32_32x32x32_i8
    // instead of 8 halves -- and only the accumulator type and the epilogue differ
    constexpr bool I8 = WQ == 88;
    static_assert(!W8 || BN == 128, "W8A16 is built for 128-wide tiles only");
    static_assert(!I8 || (BN == 128 && LD == 1), "A8W8 is built for 128-wide tiles with register-staged loaders only");
    constexpr int BM = 128, BK = 64;
    constexpr int NT = 512;
    constexpr int WN = BN / 2;   // columns per consumer wave
    constexpr int NF = WN / 32;  // 32-wide B fragments per consumer wave
    constexpr int A_BYTES = BM * BK * 2, B_BYTES = W4 ? BN * BK / 2 : W8 ? BN * BK : BN * BK * 2;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int G = W4 ? 5 : W8 ? 6 : 4 + BN / 32;      // direct loads per loader wave per stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    QV_PHASE(0);
    const bool loader = wave >= 4;
    const int w4 = wave & 3;                     // index inside the consumer / loader group
    const int wm = w4 >> 1, wn = w4 & 1;
    const int gx = gridDim.x, nwg = gridDim.x * gridDim.y;
    const int wg = xcd_tile(blockIdx.y * gx + blockIdx.x, nwg);
    const int m0 = (wg / gx) * BM, n0 = (wg % gx) * BN;

    typedef int i32x16 __attribute__((ext_vector_type(16)));
    typedef typename std::conditional<I8, i32x16, f32x16>::type acc_t;
    acc_t acc[2][NF];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    // LDS tile rows are 128 B (64 halves); the 16-B chunk index is XORed with (row >> 1) & 7 --
    // on the global SOURCE address (the direct load writes LDS lane-linearly) and on the fragment
    // read -- which spreads each ds_read_b128 lane group over all 16 slots of the 256-B bank row.
    const int nk = g.K / BK;
    auto stage = [&](int kt) {
        half_t *sA = (half_t *)(smem + (kt % NST) * STAGE_BYTES), *sB = (half_t *)((unsigned char *)sA + A_BYTES);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int chunk = w4 * 4 + q;
            int row = chunk * 8 + (lane >> 3);
            int c = (lane & 7) ^ ((row >> 1) & 7);
            int grow = m0 + row;
            grow = grow < g.M ? grow : g.M - 1;
            glds16(g.A + (size_t)grow * g.lda + kt * BK + c * 8, sA + chunk * 512);
        }
        if (W4) {
            // 64 x 64 nibble tiles are 2 KB contiguous in HBM and already swizzled: one load per 32
            // tile rows.  Every loader wave issues exactly one (with 64-wide tiles waves 2, 3 repeat
            // the loads of waves 0, 1) so that the vmcnt bookkeeping is the same for all of them.
            const int p = w4 & (BN / 32 - 1);
            glds16(g.Wq + ((size_t)((n0 >> 6) + (p >> 1)) * nk + kt) * 2048 + (p & 1) * 1024 + lane * 16,
                   (unsigned char *)sB + p * 1024);
            return;
        }
        if (W8) {
            // 64 x 64 byte tiles, 4 KB contiguous and already swizzled: two 1 KB pieces per loader wave
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int p = w4 * 2 + q;
                glds16(g.W8 + ((size_t)((n0 >> 6) + (p >> 2)) * nk + kt) * 4096 + (p & 3) * 1024 + lane * 16,
                       (unsigned char *)sB + p * 1024);
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < BN / 32; ++q) {
            int chunk = w4 * (BN / 32) + q;
            int row = chunk * 8 + (lane >> 3);
            int c = (lane & 7) ^ ((row >> 1) & 7);
            glds16(g.W + (size_t)(n0 + row) * g.ldw + kt * BK + c * 8, sB + chunk * 512);
        }
    };

    // W4: this tile's scales [K/128][BN] live in LDS behind the operand stages for the whole K loop
    half2_t *sS = (half2_t *)(smem + NST * STAGE_BYTES);   // {scale, 1024 + zero point}
    if (W4) {
        const int nkb = g.K >> 7;
        for (int idx = tid; idx < BN * nkb; idx += NT) {
            int kb = idx / BN, n = idx - kb * BN;
            sS[idx] = ((const half2_t *)g.wscale)[(size_t)kb * g.N + n0 + n];
        }
        __syncthreads();
    }

    // One raw s_barrier per K-step joins the two groups.  A loader arrives once ITS loads of stage
    // kt have landed (counted vmcnt: the loads of the younger stages stay in flight), which makes
    // the stage visible to the consumers and tells the loaders that the consumers are done with
    // stage kt - 1, whose buffer the next prefetch overwrites.  (__syncthreads() would drain the
    // whole queue and serialise the load latency with the MFMAs.)
    if (loader && LD == 1) {
        static_assert(LD == 0 || NST == 2, "register staging uses a 2-stage LDS ring");
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        constexpr int NB = W4 ? 1 : W8 ? 2 : BN / 32;   // B pieces (1 KB each) per loader wave per K-step
        constexpr int GR = 4 + NB;
        // MUBUF addressing: SGPR descriptor + per-lane 32-bit byte offset (fixed for the tile) + a scalar
        // byte offset that advances with the K-step -- no VALU instruction per load (see the header comment)
        const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)g.A, 0, (int)((size_t)g.M * g.lda * 2), 0x00020000);
        const void *bbase = W4 ? (const void *)g.Wq : W8 ? (const void *)g.W8 : I8 ? (const void *)g.Wi8 : (const void *)g.W;
        const size_t bbytes = W4 ? (size_t)g.N * g.K / 2 : W8 ? (size_t)g.N * g.K : (size_t)g.N * g.ldw * 2;
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void *)bbase, 0, (int)bbytes, 0x00020000);
        unsigned offA[4], offB[NB];
        int dstA[4], dstB[NB];
        int stepB;   // bytes between consecutive K-steps of a B piece
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int chunk = w4 * 4 + q, row = chunk * 8 + (lane >> 3), c = lane & 7;
            int grow = m0 + row;
            grow = grow < g.M ? grow : g.M - 1;
            offA[q] = (unsigned)(((size_t)grow * g.lda + c * 8) * 2);
            dstA[q] = row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
        }
        if (W4) {
            const int p = w4 & (BN / 32 - 1);
            offB[0] = (unsigned)(((size_t)((n0 >> 6) + (p >> 1)) * nk) * 2048 + (p & 1) * 1024 + lane * 16);
            dstB[0] = A_BYTES + p * 1024 + lane * 16;
            stepB = 2048;
        } else if (W8) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int p = w4 * 2 + q;
                offB[q] = (unsigned)(((size_t)((n0 >> 6) + (p >> 2)) * nk) * 4096 + (p & 3) * 1024 + lane * 16);
                dstB[q] = A_BYTES + p * 1024 + lane * 16;
            }
            stepB = 4096;
        } else {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int chunk = w4 * NB + q, row = chunk * 8 + (lane >> 3), c = lane & 7;
                offB[q] = (unsigned)(((size_t)(n0 + row) * g.ldw + c * 8) * 2);
                dstB[q] = A_BYTES + row * 128 + ((c ^ ((row >> 1) & 7)) << 4);
            }
            stepB = BK * 2;
        }
        u32x4 r0[GR], r1[GR];
        // The loads are inline asm: hipcc's own vmcnt bookkeeping merges the two register batches at the loop
        // head and drains BOTH before the first ds_write (prefetch depth 1); here the wait is counted by hand
        // -- loads return in order, so "at most GR outstanding" means the older batch has landed.
        auto fetch = [&](int kt, u32x4 (&r)[GR]) {
            if (QV_ABL(8)) return;
            const int sa = kt * (BK * 2), sb = kt * stepB;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r[q]) : "v"(offA[q]), "s"(rsA), "s"(sa) : "memory");
#pragma unroll
            for (int q = 0; q < NB; ++q)
                asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r[4 + q]) : "v"(offB[q]), "s"(rsB), "s"(sb) : "memory");
        };
        auto put = [&](int kt, const u32x4 (&r)[GR], bool newer_in_flight) {
            if (newer_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GR) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned char *st = smem + (kt % NST) * STAGE_BYTES;
            if (QV_ABL(4)) return;
#pragma unroll
            for (int q = 0; q < 4; ++q) *(u32x4 *)(st + dstA[q]) = r[q];
#pragma unroll
            for (int q = 0; q < NB; ++q) *(u32x4 *)(st + dstB[q]) = r[4 + q];
        };
        // Barrier kt: stage kt is written (loaders) and stage kt - 1 is read (consumers).  Between barriers
        // kt - 1 and kt a loader writes stage kt -- the buffer the consumers left before barrier kt - 1 --
        // out of registers that were requested two K-steps ago, then requests K-step kt + 2 into them.
        // put + fetch fused: write piece q of K-step kt, re-request it for K-step kt + 2 -- alternating stores and
        // loads keeps the LDS store path and the address path busy at the same time
        auto swap = [&](int kt, u32x4 (&r)[GR]) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GR) : "memory");   // (a newer batch is always in flight here)
            unsigned char *st = smem + (kt % NST) * STAGE_BYTES;
            const int sa = (kt + 2) * (BK * 2), sb = (kt + 2) * stepB;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!QV_ABL(4)) *(u32x4 *)(st + dstA[q]) = r[q];
                if (!QV_ABL(8)) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r[q]) : "v"(offA[q]), "s"(rsA), "s"(sa) : "memory");
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                if (!QV_ABL(4)) *(u32x4 *)(st + dstB[q]) = r[4 + q];
                if (!QV_ABL(8)) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(r[4 + q]) : "v"(offB[q]), "s"(rsB), "s"(sb) : "memory");
            }
        };
        fetch(0, r0);
        if (nk > 1) fetch(1, r1);
        for (int kt = 0; kt < nk; kt += 2) {
            int kt_ = kt;
            QV_TRACE(0);                       // barrier kt - 1 released
            if (kt + 2 < nk && QV_SWAP) swap(kt, r0);
            else { put(kt, r0, kt + 1 < nk); if (kt + 2 < nk) fetch(kt + 2, r0); }
            QV_TRACE(1);                       // (s_memtime waits lgkmcnt: loads landed + writes done)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            QV_TRACE(2);                       // arriving at barrier kt
            __builtin_amdgcn_s_barrier();
            if (kt + 1 < nk) {
                kt_ = kt + 1;
                QV_TRACE(0);
                if (kt + 3 < nk && QV_SWAP) swap(kt + 1, r1);
                else { put(kt + 1, r1, kt + 2 < nk); if (kt + 3 < nk) fetch(kt + 3, r1); }
                QV_TRACE(1);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                QV_TRACE(2);
                __builtin_amdgcn_s_barrier();
            }
        }
    } else if (loader) {
#pragma unroll
        for (int s = 0; s < NST - 1; ++s)
            if (s < nk) stage(s);
        for (int kt = 0; kt < nk; ++kt) {
            const int ahead = min(nk - 1 - kt, NST - 2);  // stages issued after stage kt
            if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * G) : "memory");
            else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (kt + NST - 1 < nk) stage(kt + NST - 1);
        }
    }
    for (int kt = 0; kt < (loader ? 0 : nk); ++kt) {
        const int kt_ = kt;
        QV_TRACE(2);                           // arriving at barrier kt (K-step kt - 1 computed)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt == 0) QV_PHASE(1);
        QV_TRACE(0);                           // barrier kt released
        const half_t *sA = (const half_t *)(smem + (kt % NST) * STAGE_BYTES);
        const half_t *sB = (const half_t *)((const unsigned char *)sA + A_BYTES);
        half2_t sc[NF], zo[NF];
        if (W4) {
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                half2_t sz = sS[(kt >> 1) * BN + wn * WN + j * 32 + (lane & 31)];
                sc[j] = half2_t{sz[0], sz[0]};
                zo[j] = half2_t{sz[1], sz[1]};
            }
        }
        // Fragment reads are software-pipelined over the four 16-deep sub-steps: the reads of sub-step ks + 1
        // are in flight while the MFMAs of sub-step ks run (two register sets).  With one set the next reads
        // could only issue behind the last MFMA of a sub-step and every sub-step exposed one LDS latency
        // (~90 of ~220 cycles, tools/gemm_trace.hip: 964 cycles per K-step for 512 cycles of MFMA).
        struct Raw { half8 a[2]; half8 b[NF]; uint32_t q4[NF]; uint2 q8[NF]; };
        auto rd = [&](int ks, Raw &f) {
            if (QV_ABL(2)) return;
            const int c = ks * 2 + (lane >> 5);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wm * 64 + i * 32 + (lane & 31);
                f.a[i] = *(const half8 *)(sA + row * 64 + ((c ^ ((row >> 1) & 7)) << 3));
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const int row = wn * WN + j * 32 + (lane & 31);
                if (W4) {
                    // 32-byte rows, 4-byte chunks at c ^ ((row >> 2) & 7): the 64 lanes of the
                    // ds_read_b32 hit 64 different banks
                    f.q4[j] = *(const uint32_t *)((const unsigned char *)sB + row * 32 + ((c ^ ((row >> 2) & 7)) << 2));
                } else if (W8) {
                    // 64-byte rows, 8-byte chunks at c ^ ((row >> 2) & 7); bytes are q + 128
                    f.q8[j] = *(const uint2 *)((const unsigned char *)sB + (row >> 6) * 4096 + (row & 63) * 64 +
                                               ((c ^ ((row >> 2) & 7)) << 3));
                } else {
                    f.b[j] = *(const half8 *)(sB + row * 64 + ((c ^ ((row >> 1) & 7)) << 3));
                }
            }
        };
        auto mma = [&](const Raw &f) {
            if (QV_ABL(1)) {
#pragma unroll
                for (int i = 0; i < 2; ++i) asm volatile("" ::"v"(f.a[i]));
#pragma unroll
                for (int j = 0; j < NF; ++j) { asm volatile("" ::"v"(f.b[j])); asm volatile("" ::"v"(f.q4[j])); asm volatile("" ::"v"(f.q8[j])); }
                return;
            }
            half8 b[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j) b[j] = W4 ? dequant8(f.q4[j], sc[j], zo[j]) : W8 ? dequant8_i8(f.q8[j]) : f.b[j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) {
                    // operands swapped (D^T = W A^T): a lane holds 4 CONSECUTIVE output columns per
                    // register quad -> 8/16-byte LDS writes in the epilogue
                    if constexpr (I8)
                        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, b[j]), __builtin_bit_cast(i32x4, f.a[i]),
                                                                          acc[i][j], 0, 0, 0);
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[j], f.a[i], acc[i][j], 0, 0, 0);
                }
        };
        // (sched_barrier: left alone, the scheduler sinks every read group back behind the previous MFMAs
        // to save the 16 registers)
        Raw f0 = {}, f1 = {};
        rd(0, f0);
        rd(1, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(f0);
        __builtin_amdgcn_sched_barrier(0);
        rd(2, f0);
        __builtin_amdgcn_sched_barrier(0);
        mma(f1);
        __builtin_amdgcn_sched_barrier(0);
        rd(3, f1);
        __builtin_amdgcn_sched_barrier(0);
        mma(f0);
        __builtin_amdgcn_sched_barrier(0);
        mma(f1);
    }
    __syncthreads();  // every wave is done with the operand stages before the epilogue reuses them
    QV_PHASE(2);
#if defined(QV_GEMM_TRACE) && defined(__HIP_DEVICE_COMPILE__)
    if (QV_ABL(32)) {   // no epilogue at all (accumulators kept live)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) asm volatile("" ::"v"(acc[i][j]));
        return;
    }
#endif

    // ------------------------------------------------------------------ epilogue ----------
    // accumulator (i, j), register r: tile row  = wm*64 + i*32 + (lane & 31),
    //   tile column = wn*WN + j*32 + 8*(r >> 2) + 4*(lane >> 5) + (r & 3)
    const int l31 = lane & 31, hi = lane >> 5;
    // Every global access of the epilogue goes through MUBUF (SGPR descriptor + 32-bit byte offset): while the
    // co-resident block's consumer waves keep the SIMDs' matrix pipes busy, FLAT-encoded loads and stores of
    // this block would wait for a gap in their MFMA stream (see the LD = 1 note above).
    typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rs_bias = __builtin_amdgcn_make_buffer_rsrc((void *)g.bias, 0, g.N * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_scl = __builtin_amdgcn_make_buffer_rsrc((void *)(W8 ? g.w8scale : g.bias), 0, g.N * 4, 0x00020000);
    auto ldf4 = [&](const __amdgpu_buffer_rsrc_t &rs, int elem) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, elem * 4, 0, 0));
    };

    if constexpr (I8) {
        // ---- A8W8 epilogue (val_a8w8): the whole tile is staged as float32, ranges folded block-wide
        constexpr bool GLU = A8W8<EPI>::GLU, OUT16 = A8W8<EPI>::OUT16, RELU = A8W8<EPI>::RELU, FOLD = A8W8<EPI>::FOLD;
        constexpr int BNO = GLU ? BN / 2 : BN;
        constexpr int LDT = BNO + 4;                                   // floats per staged row
        float *sO = (float *)smem;
        uint32_t *sMM = (uint32_t *)(smem + BM * LDT * 4);             // [BM][2] range keys of the tile's rows
        if (FOLD) {
            for (int k = tid; k < BM * 2; k += NT) sMM[k] = (k & 1) ? 0u : 0xFFFFFFFFu;   // empty range
            __syncthreads();
        }
        if (!loader) {
            const __amdgpu_buffer_rsrc_t rs_ws = __builtin_amdgcn_make_buffer_rsrc((void *)g.wsum, 0, g.N * 4, 0x00020000);
            float srow[2];
            int zc[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int grow = m0 + wm * 64 + i * 32 + l31;
                grow = grow < g.M ? grow : g.M - 1;
                bool valid;
                a8w8_row_param(g, row_owner(g, grow, valid), srow[i], zc[i]);
            }
            float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
            if (GLU) {
                // W rows interleaved in 32-channel groups: [value(32) | gate(32)] per 64 columns
                const int nb = n0 + wn * WN;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int nl = 8 * q + 4 * hi;
                    const f32x4 ba = ldf4(rs_bias, nb + nl), bg = ldf4(rs_bias, nb + 32 + nl);
                    const i32x4 wa = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_ws, (nb + nl) * 4, 0, 0));
                    const i32x4 wg = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_ws, (nb + 32 + nl) * 4, 0, 0));
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int rl = wm * 64 + i * 32 + l31;
                        f32x4 o, av, gv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            av[e] = val_a8w8<false>(acc[i][0][q * 4 + e], zc[i], wa[e], srow[i], ba[e]);
                            gv[e] = val_a8w8<false>(acc[i][NF - 1][q * 4 + e], zc[i], wg[e], srow[i], bg[e]);
                        }
                        const f32x4 sg = sigmoid4(gv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { o[e] = av[e] * sg[e]; track(o[e], mn[i], mx[i]); }
                        *(f32x4 *)(sO + rl * LDT + wn * (WN / 2) + nl) = o;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NF; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cl = wn * WN + j * 32 + 8 * q + 4 * hi;
                        const f32x4 bb = ldf4(rs_bias, n0 + cl);
                        const i32x4 ws = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_ws, (n0 + cl) * 4, 0, 0));
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const int rl = wm * 64 + i * 32 + l31;
                            f32x4 o;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                o[e] = val_a8w8<RELU>(acc[i][j][q * 4 + e], zc[i], ws[e], srow[i], bb[e]);
                                track(o[e], mn[i], mx[i]);
                            }
                            *(f32x4 *)(sO + rl * LDT + cl) = o;
                        }
                    }
            }
            if (FOLD) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int rl = wm * 64 + i * 32 + l31;
                    atomicMin(&sMM[2 * rl], fenc(mn[i]));
                    atomicMax(&sMM[2 * rl + 1], fenc(mx[i]));
                }
            }
        }
        __syncthreads();
        if (FOLD) {
            // One atomic pair per (tile, utterance), not per row: all tiles start at once and every row's pair would
            // land on its utterance's two addresses (measured: 200 us for this GEMM instead of 15).  A tile's rows are
            // sorted by utterance, so the first row of each run reduces the run.
            int *sU = (int *)(sMM + 2 * BM);       // [BM] owner of each row, -1 = not a valid row
            if (tid < BM) {
                bool valid = false;
                int u = -1;
                if (m0 + tid < g.M) u = row_owner(g, m0 + tid, valid);
                sU[tid] = valid && sMM[2 * tid] <= sMM[2 * tid + 1] ? u : -1;
            }
            __syncthreads();
            if (tid < BM && sU[tid] >= 0 && (tid == 0 || sU[tid - 1] != sU[tid])) {
                uint32_t kn = sMM[2 * tid], kx = sMM[2 * tid + 1];
                for (int k = tid + 1; k < BM && sU[k] == sU[tid]; ++k) { kn = min(kn, sMM[2 * k]); kx = max(kx, sMM[2 * k + 1]); }
                mm_fold_keys(g.mm_out + QV_MM_STRIDE * sU[tid], kn, kx);
            }
        }
        // the output descriptor is rebased on this tile's first row: the dense subsampling tensors have millions of rows
        // (4-byte elements), and a whole-tensor descriptor would need more than its 32-bit size / offsets hold
        const int tile_rows = g.M - m0 < BM ? g.M - m0 : BM;
        if (OUT16) {
            constexpr int CPR = BNO / 8;   // 16-byte chunks of halves per row
            const __amdgpu_buffer_rsrc_t rs_out16 = __builtin_amdgcn_make_buffer_rsrc((half_t *)g.out + (size_t)m0 * g.ldo, 0,
                                                                                      tile_rows * g.ldo * 2, 0x00020000);
            for (int idx = tid; idx < BM * CPR; idx += NT) {
                const int r = idx / CPR, c = (idx % CPR) * 8;
                if (r >= tile_rows) continue;
                const f32x4 a = *(const f32x4 *)(sO + r * LDT + c), b = *(const f32x4 *)(sO + r * LDT + c + 4);
                const half8 h = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3], (half_t)b[0], (half_t)b[1], (half_t)b[2], (half_t)b[3]};
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, h), rs_out16, (r * g.ldo + n0 + c) * 2, 0, 0);
            }
        } else {
            constexpr int CPR = BNO / 4;            // 16-byte chunks per row
            constexpr int IT = BM * CPR / NT;       // chunks per thread (exact)
            const int n0o = GLU ? n0 / 2 : n0;
            const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((float *)g.out + (size_t)m0 * g.ldo, 0,
                                                                                    tile_rows * g.ldo * 4, 0x00020000);
            f32x4 old[IT];
            if (EPI == EPI_RESID) {
#pragma unroll
                for (int k = 0; k < IT; ++k) {
                    const int idx = tid + k * NT, r = idx / CPR, c = (idx % CPR) * 4;
                    if (r < tile_rows) old[k] = ldf4(rs_out, r * g.ldo + n0o + c);
                }
            }
#pragma unroll
            for (int k = 0; k < IT; ++k) {
                const int idx = tid + k * NT, r = idx / CPR, c = (idx % CPR) * 4;
                if (r >= tile_rows) continue;
                f32x4 v = *(const f32x4 *)(sO + r * LDT + c);
                if (EPI == EPI_RESID) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = a8w8_resid(old[k][e], g.alpha, v[e]);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs_out, (r * g.ldo + n0o + c) * 4, 0, 0);
            }
        }
        return;
    }

    if (EPI == EPI_QKV && n0 >= 2 * QV_D) {
        // V tile: stored TRANSPOSED, Vt[b][h*64+d][t].  The tile goes through LDS as [d][frame] so
        // that all 8 waves write it out with the 64 lanes of a store on 128 consecutive frames of
        // one d (4-byte pairs, 256 B per instruction); stores straight from the accumulator layout
        // (2-byte elements, 32 frames per d) cost 8 us per GEMM.
        constexpr int LDV = BM + 2;   // halves per d row (odd dword pitch: d rows rotate over the banks)
        half_t *sT = (half_t *)smem;
        if (!loader) {
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = wn * WN + j * 32 + 8 * q + 4 * hi;
                    const f32x4 bb = ldf4(rs_bias, n0 + cl);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int rl = wm * 64 + i * 32 + l31;
#pragma unroll
                        for (int e = 0; e < 4; ++e) sT[(cl + e) * LDV + rl] = val_v(acc[i][j][q * 4 + e], bb[e]);
                    }
                }
        }
        __syncthreads();
        // thread -> frame pair (fixed), then d = tid / 64 + 8 k
        const int r0 = m0 + 2 * lane, r1 = r0 + 1;
        const int bt0 = r0 < g.M ? g.row_map[r0] : -1, bt1 = r1 < g.M ? g.row_map[r1] : -1;
        const bool pair = bt0 >= 0 && bt1 == bt0 + 1 && (bt0 & 1) == 0;   // same utterance, even frame: one 4-byte store
        half_t *vt = (half_t *)g.out2;
        for (int d = wave; d < BN; d += NT / 64) {
            const size_t drow = (size_t)(n0 - 2 * QV_D + d);
            const half_t v0 = sT[d * LDV + 2 * lane], v1 = sT[d * LDV + 2 * lane + 1];
            if (pair) {
                half2_t v = {v0, v1};
                *(half2_t *)(vt + vt_index(g, bt0, drow)) = v;
            } else {
                if (bt0 >= 0) vt[vt_index(g, bt0, drow)] = v0;
                if (bt1 >= 0) vt[vt_index(g, bt1, drow)] = v1;
            }
        }
        QV_PHASE(3);
        return;
    }

    // this wave's bias values, requested together (g.bias is never null: one load latency, not
    // one per register quad)
    f32x4 bia[NF][4], scl[NF][4];   // scl: per-channel weight scales (W8A16 only)
    if (EPI != EPI_GLU && !loader) {
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bia[j][q] = ldf4(rs_bias, n0 + wn * WN + j * 32 + 8 * q + 4 * hi);
                if (W8) scl[j][q] = ldf4(rs_scl, n0 + wn * WN + j * 32 + 8 * q + 4 * hi);
            }
    }

    if (out_is_f32(EPI)) {
        constexpr int LDT = BN + 4;  // floats per staged row (pad keeps 16-B alignment)
        float *sO = (float *)smem;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (loader) continue;   // only the consumer waves hold accumulators
            const int rl = wm * 64 + i * 32 + l31;
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = wn * WN + j * 32 + 8 * q + 4 * hi;
                    f32x4 v;
                    const f32x4 bb = bia[j][q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = val_f32<W8>(acc[i][j][q * 4 + e], W8 ? scl[j][q][e] : 1.f, g.alpha, bb[e]);
                    *(f32x4 *)(sO + rl * LDT + cl) = v;
                }
        }
        __syncthreads();
        constexpr int CPR = BN / 4;            // 16-byte chunks per row
        constexpr int IT = BM * CPR / NT;      // chunks per thread (exact)
        // residual: all of a thread's old values are requested before the first store (a store
        // followed by the next load of the same array would serialise one latency per chunk)
        f32x4 old[IT];
        // (the descriptor's size bounds the rows: loads past row M return 0, stores past it are dropped)
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(g.out, 0, (int)((size_t)g.M * g.ldo * 4), 0x00020000);
        if (EPI == EPI_RESID) {
#pragma unroll
            for (int k = 0; k < IT; ++k) {
                int idx = tid + k * NT, r = idx / CPR, c = (idx % CPR) * 4;
                if (m0 + r < g.M && !QV_ABL(16)) old[k] = ldf4(rs_out, (m0 + r) * g.ldo + n0 + c);
            }
        }
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            int idx = tid + k * NT, r = idx / CPR, c = (idx % CPR) * 4;
            if (m0 + r >= g.M) continue;
            f32x4 v = *(const f32x4 *)(sO + r * LDT + c);
            if (EPI == EPI_RESID) add_resid(v, old[k]);
            if (QV_ABL(16)) { asm volatile("" ::"v"(v)); continue; }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs_out, ((m0 + r) * g.ldo + n0 + c) * 4, 0, 0);
        }
        QV_PHASE(3);
        return;
    }

    {
        constexpr int BNO = EPI == EPI_GLU ? BN / 2 : BN;  // output tile width
        constexpr int LDT = BNO + 8;                        // halves per staged row
        half_t *sO = (half_t *)smem;
        const int n0o = EPI == EPI_GLU ? n0 / 2 : n0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (loader) continue;   // only the consumer waves hold accumulators
            const int rl = wm * 64 + i * 32 + l31;
            if (EPI == EPI_GLU) {
                // W rows interleaved in 32-channel groups: [value(32) | gate(32)] per 64 columns
                const int nb = n0 + wn * WN;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int nl = 8 * q + 4 * hi;
                    f32x4 ba = ldf4(rs_bias, nb + nl), bg = ldf4(rs_bias, nb + 32 + nl);
                    f32x4 sa = {1.f, 1.f, 1.f, 1.f}, sg = sa;
                    if (W8) { sa = ldf4(rs_scl, nb + nl); sg = ldf4(rs_scl, nb + 32 + nl); }
                    *(half4 *)(sO + rl * LDT + wn * (WN / 2) + nl) = val_glu<W8>(acc[i][0], acc[i][NF - 1], q, sa, sg, ba, bg);
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cl = wn * WN + j * 32 + 8 * q + 4 * hi;
                    const f32x4 bb = bia[j][q];
                    *(half4 *)(sO + rl * LDT + cl) = val_f16<EPI>(acc[i][j], q, bb);
                }
        }
        __syncthreads();
        constexpr int CPR = BNO / 8;  // 16-byte chunks per row
        const __amdgpu_buffer_rsrc_t rs_out16 = __builtin_amdgcn_make_buffer_rsrc(g.out, 0, (int)((size_t)g.M * g.ldo * 2), 0x00020000);
        for (int idx = tid; idx < BM * CPR; idx += NT) {
            int r = idx / CPR, c = (idx % CPR) * 8;
            if (m0 + r >= g.M) continue;
            if (QV_ABL(16)) { asm volatile("" ::"v"(*(const half8 *)(sO + r * LDT + c))); continue; }
            __builtin_amdgcn_raw_buffer_store_b128(*(const u32x4_t *)(sO + r * LDT + c), rs_out16, ((m0 + r) * g.ldo + n0o + c) * 2, 0, 0);
        }
        QV_PHASE(3);
    }
#undef QV_TRACE
