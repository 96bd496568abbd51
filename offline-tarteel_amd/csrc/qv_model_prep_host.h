// qv_model_prep_host.h -- from the named tensors of a weight source (qv_weights_host.h) to the images the kernels read:
// every layout decision the forward relies on (tap-major stencils, the permuted pre_encode.out, the padded head, Q/K/V
// and linear_pos fused along N, the GLU pairing, BatchNorm folded or kept as alpha / beta, the quantised forms of
// qv_wpack_host.h and of the ORT precision).  HIP-free (the standard library only): the half type is the including
// file's, `typedef _Float16 half_t;` in front of this header (qv_kernels.h in the library).  An image leaves through a
// caller-supplied sink, `template <class T> int sink(const std::vector<T> &image, const T **slot)`: the library's sink
// (qv_model.hip) makes one device allocation per image, in the order of the calls; HostSink below keeps the images on
// the host, which is how tools/weight_prep_check.cpp runs all of this under ASan + UBSan on a machine without a GPU.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "qv_limits.h"
#include "qv_weights_host.h"   // HostWeights, QvMissingWeight
#include "qv_wpack_host.h"     // qv_pack_w4, qv_pack_w4_given, qv_pack_w8

#define N_LAYERS QV_N_LAYERS
#define HEAD_N 1152  // 1025 padded to a multiple of 128

#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// one GEMM weight matrix: f16 [N][K], or (int4 mode, Linear layers) packed nibbles + f16 scales
struct WMat {
    const half_t *w = nullptr;
    const uint8_t *q = nullptr;
    const half_t *sc = nullptr;
    const uint8_t *q8 = nullptr;   // int8 mode (pointwise convolutions): packed q + 128 ...
    const float *sc8 = nullptr;    // ... and the per-output-channel scales
};

// QV_PREC_ORT_MIXED: a Conv weight as quantize_dynamic(QInt8) stores it -- ONE symmetric scale per tensor
struct OrtConv {                   // GEMM-shaped (1x1) convolution: s8 [N][K] row-major + the row sums the epilogue needs
    const int8_t *wq = nullptr;
    const int32_t *wsum = nullptr;
    float scale = 1.f;
};
struct OrtDw {                     // depthwise / strided convolution: taps as integer-valued floats, tap-major [9][C]
    const float *wq = nullptr;
    float scale = 1.f;
};

struct LayerW {
    const float *ln_g[5], *ln_b[5];  // ff1, att, conv, ff2, out
    WMat ff1_w1, ff1_w2, ff2_w1, ff2_w2, qkv_w, out_w, pw1_w, pw2_w;
    const float *ff1_b1, *ff1_b2, *ff2_b1, *ff2_b2, *qkv_b, *out_b, *pw1_b, *pw2_b;
    const float *bias_u, *bias_v, *dw_w, *dw_b;
    // QV_PREC_ORT_MIXED
    OrtConv o_pw1, o_pw2;
    OrtDw o_dw;
    const float *o_dw_b, *bn_alpha, *bn_beta;   // raw depthwise bias; BatchNorm as torch evaluates it: fma(y, alpha, beta)
};

// every weight image of the model: the description the forward schedule reads and the prepared-image checks dump
struct ModelW {
    // front-end tables (FrontendTab in qv_layers.h, field for field)
    const float *window;     // [512] symmetric Hann(400) zero-padded to n_fft, centred
    const float *twiddle;    // [256][2] exp(-2 pi i m / 512) as {re, im}: the float2 array k_logmel reads
    const int32_t *mel_lo;   // [80] first FFT bin of each filter
    const int32_t *mel_cnt;  // [80] number of bins (<= 32)
    const float *mel_w;      // [32][80]: tap-major (tap k of filter m at k * 80 + m), zero beyond a filter's mel_cnt
    const float *c0_w, *c0_b, *dw2_w, *dw2_b, *dw5_w, *dw5_b, *pw3_b, *pw6_b, *sub_out_b, *head_b;
    const half_t *pw3_w, *pw6_w, *sub_out_w, *head_w;
    WMat pos_w;
    const float *zero_bias;
    OrtDw o_c0, o_dw2, o_dw5;
    OrtConv o_pw3, o_pw6, o_head;
    LayerW L[N_LAYERS];
    int prequant_w4_linears = 0, prequant_f16_linears = 0;   // a pre-quantised file's Linear weights on the file's int4 grid / as f16 values
};

// the sink of a host-only run: keeps every image alive and hands back its data()
struct HostSink {
    struct Image { std::shared_ptr<void> keep; const void *data; size_t bytes; };
    std::vector<Image> images;   // in the order of the calls
    template <class T>
    int operator()(const std::vector<T> &image, const T **slot) {
        auto keep = std::make_shared<std::vector<T>>(image);
        images.push_back({keep, keep->data(), keep->size() * sizeof(T)});
        *slot = keep->data();
        return QV_OK;
    }
};

// [C][9] -> [9][C] (tap-major) so a thread's 8 channels of one tap are one 32-byte load
inline std::vector<float> tap_major(const std::vector<float> &w, int C) {
    std::vector<float> t((size_t)C * 9);
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < 9; ++k) t[(size_t)k * C + c] = w[(size_t)c * 9 + k];
    return t;
}

inline std::vector<half_t> to_half(const std::vector<float> &v) {
    std::vector<half_t> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = (half_t)v[i];
    return h;
}

// MatMulNBits' symmetric block-128 int4 (qv_pack_w4's rule: scale = the block's extreme value / -8, zero point 8) with
// the FLOAT32 scale: w <- (q - 8) * scale in place -- oracle/fastconformer_ref.py::quant_dequant_int4_f32scale
inline void int4_quant_dequant(std::vector<float> &w, int N, int K) {
    for (int n = 0; n < N; ++n)
        for (int kb = 0; kb < K / 128; ++kb) {
            float *blk = w.data() + (size_t)n * K + kb * 128;
            float vmax = 0.f, amax = -1.f;
            for (int k = 0; k < 128; ++k) {
                float a = fabsf(blk[k]);
                if (a > amax) { amax = a; vmax = blk[k]; }
            }
            const float scale = vmax / -8.0f, rs = scale != 0.f ? 1.0f / scale : 0.f;
            for (int k = 0; k < 128; ++k) {
                int q = (int)floorf(blk[k] * rs + 8.5f);
                q = q < 0 ? 0 : q > 15 ? 15 : q;
                blk[k] = ((float)q - 8.0f) * scale;
            }
        }
}

// quantize_dynamic(weight_type = QInt8) on one Conv weight tensor: scale = max|w| / 127 (the division in double, the
// result rounded to float32), q = saturate(round-half-even(w / scale)) -- oracle/fastconformer_ref.py::quantize_weight_int8
// `given` > 0: the scale a pre-quantised file stored for this tensor (w = q * given exactly, so q comes back verbatim).
inline float quant_w8_tensor(const std::vector<float> &w, std::vector<int8_t> &q, float given = 0.f) {
    float amax = 0.f;
    for (float v : w) amax = std::max(amax, fabsf(v));
    const float sw = given > 0.f ? given : amax > 0.f ? (float)((double)amax / 127.0) : 1.0f;
    q.resize(w.size());
    for (size_t i = 0; i < w.size(); ++i) {
        float t = nearbyintf(w[i] / sw);   // default rounding mode: half to even
        t = t < -127.f ? -127.f : t > 127.f ? 127.f : t;
        q[i] = (int8_t)t;
    }
    return sw;
}

// One preparation run: the precision (w4: Linear-layer weights are block-128 int4; ort: every Conv runs
// DynamicQuantizeLinear -> ConvInteger; prequant: the source is marked pre-quantised and nothing is re-quantised), the
// sink, the images' slots.  A refusal leaves its text in `err`; HostWeights::get throws QvMissingWeight through all of it.
template <class Sink>
struct WeightPrep {
    Sink &sink;
    const bool w4, ort, prequant;
    ModelW &mw;
    std::string &err;
    std::vector<float> gs_tmp, gz_tmp;   // grid_of's concatenation

    template <typename T>
    int up(const std::vector<T> &h, const T **dev) { return sink(h, dev); }

    // upload a Linear weight [N][K]: f16, or int4 nibbles + scales when the model runs W4A16.  A pre-quantised file's weight
    // goes onto the FILE's grid (`gs`, `gz`: its block scales / zero points) and is never re-quantised; without a grid
    // (MatMulNBits block size other than 128) it runs as its dequantised values, f16.
    int up_mat(const std::vector<float> &w, int N, int K, WMat *out, const std::vector<float> *gs = nullptr,
               const std::vector<float> *gz = nullptr) {
        const bool grid = prequant && gs && gz && gs->size() == (size_t)N * (K / 128) && gz->size() == gs->size();
        if (!w4 || (prequant && !grid)) {
            if (w4) ++mw.prequant_f16_linears;
            return up(to_half(w), &out->w);
        }
        std::vector<uint8_t> q((size_t)N * K / 2, 0);
        std::vector<half_t> sc((size_t)N * (K / 128) * 2);
        if (grid) {
            const int64_t bad = qv_pack_w4_given(w.data(), N, K, gs->data(), gz->data(), q.data(), sc.data());
            if (bad) { err = "pre-quantised weight file: a Linear weight does not sit on the int4 grid it declares (or a block has a non-integer zero point / a scale outside f16's normal range)"; return QV_ERR_IO; }
            ++mw.prequant_w4_linears;
        } else
        qv_pack_w4(w.data(), N, K, q.data(), sc.data());
        TRY(up(q, &out->q));
        return up(sc, &out->sc);
    }

    // upload a pointwise-convolution weight [N][K]: f16, or per-channel int8 when the model runs mixed
    int up_mat8(const std::vector<float> &w, int N, int K, WMat *out) {
        if (ort) return QV_OK;   // (the A8W8 operands are prepared by up_ort_conv)
        if (!w4 || prequant) return up(to_half(w), &out->w);
        std::vector<uint8_t> q((size_t)N * K, 0);
        std::vector<float> sc((size_t)N);
        qv_pack_w8(w.data(), N, K, q.data(), sc.data());
        TRY(up(q, &out->q8));
        return up(sc, &out->sc8);
    }

    // GEMM-shaped convolution weight [N][K] (rows past n_valid are zero padding): s8 row-major, row sums, scale
    int up_ort_conv(const std::vector<float> &w, int n_valid, int N, int K, OrtConv *out, float given = 0.f) {
        std::vector<int8_t> q;
        out->scale = quant_w8_tensor(w, q, given);
        std::vector<int8_t> qp((size_t)N * K, 0);
        std::vector<int32_t> ws(N, 0);
        for (int n = 0; n < n_valid; ++n) {
            int32_t sum = 0;
            for (int k = 0; k < K; ++k) { qp[(size_t)n * K + k] = q[(size_t)n * K + k]; sum += q[(size_t)n * K + k]; }
            ws[n] = sum;
        }
        TRY(up(qp, &out->wq));
        return up(ws, &out->wsum);
    }

    // depthwise weight [C][9]: integer-valued floats, tap-major [9][C]
    int up_ort_dw(const std::vector<float> &w, int C, OrtDw *out, float given = 0.f) {
        std::vector<int8_t> q;
        out->scale = quant_w8_tensor(w, q, given);
        std::vector<float> t((size_t)C * 9);
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < 9; ++k) t[(size_t)k * C + c] = (float)q[(size_t)c * 9 + k];
        return up(t, &out->wq);
    }

    int build_frontend() {
        // symmetric Hann(400) centred in 512
        std::vector<float> win(512, 0.f);
        for (int i = 0; i < 400; ++i) win[56 + i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / 399.0));
        std::vector<float> tw(2 * 256);
        for (int k = 0; k < 256; ++k) { tw[2 * k] = (float)cos(-2.0 * M_PI * k / 512.0); tw[2 * k + 1] = (float)sin(-2.0 * M_PI * k / 512.0); }
        // Slaney mel filterbank (librosa.filters.mel, htk=False, norm='slaney'), f64 then f32
        auto hz_to_mel = [](double f) {
            const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = 1000.0 / f_sp, logstep = log(6.4) / 27.0;
            return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
        };
        auto mel_to_hz = [](double mm) {
            const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = 1000.0 / f_sp, logstep = log(6.4) / 27.0;
            return mm >= min_log_mel ? min_log_hz * exp(logstep * (mm - min_log_mel)) : f_sp * mm;
        };
        double mlo = hz_to_mel(0.0), mhi = hz_to_mel(8000.0);
        std::vector<double> mel_f(QV_NMEL + 2);
        for (int i = 0; i < QV_NMEL + 2; ++i) mel_f[i] = mel_to_hz(mlo + (mhi - mlo) * i / (QV_NMEL + 1));
        std::vector<int32_t> lo(QV_NMEL), cnt(QV_NMEL);
        std::vector<float> w(QV_NMEL * 32, 0.f);
        for (int i = 0; i < QV_NMEL; ++i) {
            double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
            int first = -1, last = -1;
            std::vector<float> row(257);
            for (int k = 0; k < 257; ++k) {
                double fk = 8000.0 * k / 256.0;
                double lower = (fk - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
                double upper = (mel_f[i + 2] - fk) / (mel_f[i + 2] - mel_f[i + 1]);
                double v = std::max(0.0, std::min(lower, upper));
                row[k] = (float)(v * enorm);
                if (row[k] > 0.f) { if (first < 0) first = k; last = k; }
            }
            if (first < 0) { first = 0; last = 0; }
            if (last - first + 1 > 32) { err = "mel filter wider than 32 bins"; return QV_ERR_ARG; }
            lo[i] = first; cnt[i] = last - first + 1;
            // tap-major [32][80]: the lanes of k_logmel's projection are consecutive filters reading the same tap, so a
            // wave's load is 320 contiguous bytes (filter-major, every lane hit its own cache line: 64 lines per load)
            for (int k = first; k <= last; ++k) w[(size_t)(k - first) * QV_NMEL + i] = row[k];
        }
        TRY(up(win, &mw.window));
        TRY(up(tw, &mw.twiddle));
        TRY(up(lo, &mw.mel_lo));
        TRY(up(cnt, &mw.mel_cnt));
        TRY(up(w, &mw.mel_w));
        return QV_OK;
    }

    // the subsampling stack and the CTC head
    int prepare_front(const HostWeights &hw) {
        const std::string pe = "encoder.pre_encode.";
        TRY(up(tap_major(hw.get(pe + "conv.0.weight"), QV_SUBC), &mw.c0_w));
        TRY(up(hw.get(pe + "conv.0.bias"), &mw.c0_b));
        TRY(up(tap_major(hw.get(pe + "conv.2.weight"), QV_SUBC), &mw.dw2_w));
        TRY(up(hw.get(pe + "conv.2.bias"), &mw.dw2_b));
        TRY(up(to_half(hw.get(pe + "conv.3.weight")), &mw.pw3_w));
        TRY(up(hw.get(pe + "conv.3.bias"), &mw.pw3_b));
        TRY(up(tap_major(hw.get(pe + "conv.5.weight"), QV_SUBC), &mw.dw5_w));
        TRY(up(hw.get(pe + "conv.5.bias"), &mw.dw5_b));
        TRY(up(to_half(hw.get(pe + "conv.6.weight")), &mw.pw6_w));
        TRY(up(hw.get(pe + "conv.6.bias"), &mw.pw6_b));
        if (ort) {
            TRY(up_ort_dw(hw.get(pe + "conv.0.weight"), QV_SUBC, &mw.o_c0, hw.int8_scale(pe + "conv.0.weight")));
            TRY(up_ort_dw(hw.get(pe + "conv.2.weight"), QV_SUBC, &mw.o_dw2, hw.int8_scale(pe + "conv.2.weight")));
            TRY(up_ort_dw(hw.get(pe + "conv.5.weight"), QV_SUBC, &mw.o_dw5, hw.int8_scale(pe + "conv.5.weight")));
            TRY(up_ort_conv(hw.get(pe + "conv.3.weight"), QV_SUBC, QV_SUBC, QV_SUBC, &mw.o_pw3, hw.int8_scale(pe + "conv.3.weight")));
            TRY(up_ort_conv(hw.get(pe + "conv.6.weight"), QV_SUBC, QV_SUBC, QV_SUBC, &mw.o_pw6, hw.int8_scale(pe + "conv.6.weight")));
            TRY(up_ort_conv(hw.get("ctc_decoder.decoder_layers.0.weight"), QV_VOCAB, HEAD_N, QV_D, &mw.o_head,
                            hw.int8_scale("ctc_decoder.decoder_layers.0.weight")));
        }
        {
            // Linear(2560 -> 512): NeMo flattens [C=256][F=10] as c*10+f; activations here are
            // channels-last [F][C], so permute K to f*256+c
            std::vector<float> w = hw.get(pe + "out.weight");
            if (ort && !prequant) {
                // MatMulNBits quantises along the ORIGINAL K order (blocks of 128 consecutive c*10+f); the permuted layout
                // no longer has those blocks, so this one Linear is quantised -> dequantised here and runs as an f16 GEMM
                // on exactly the values (q - 8) * scale
                int4_quant_dequant(w, QV_D, 2560);
            }
            std::vector<half_t> p((size_t)QV_D * 2560);
            for (int n = 0; n < QV_D; ++n)
                for (int c = 0; c < QV_SUBC; ++c)
                    for (int f = 0; f < 10; ++f) p[(size_t)n * 2560 + f * QV_SUBC + c] = (half_t)w[(size_t)n * 2560 + c * 10 + f];
            TRY(up(p, &mw.sub_out_w));
            TRY(up(hw.get(pe + "out.bias"), &mw.sub_out_b));
        }
        {
            const std::vector<float> &w = hw.get("ctc_decoder.decoder_layers.0.weight");
            const std::vector<float> &b = hw.get("ctc_decoder.decoder_layers.0.bias");
            std::vector<half_t> p((size_t)HEAD_N * QV_D, (half_t)0.f);
            std::vector<float> pb(HEAD_N, 0.f);
            for (size_t i = 0; i < (size_t)QV_VOCAB * QV_D; ++i) p[i] = (half_t)w[i];
            for (int i = 0; i < QV_VOCAB; ++i) pb[i] = b[i];
            TRY(up(p, &mw.head_w));
            TRY(up(pb, &mw.head_b));
        }
        return QV_OK;
    }

    // the file's own int4 grid of a Linear weight (pre-quantised files only), concatenated along N for fused weights
    void grid_of(const HostWeights &hw, std::initializer_list<std::string> names, const std::vector<float> *&gs, const std::vector<float> *&gz) {
        gs = gz = nullptr;
        if (!prequant) return;
        gs_tmp.clear(); gz_tmp.clear();
        for (const std::string &n : names) {
            const std::vector<float> *a = hw.int4_scale(n), *b = hw.int4_zp(n);
            if (!a || !b || a->size() != b->size()) return;
            gs_tmp.insert(gs_tmp.end(), a->begin(), a->end());
            gz_tmp.insert(gz_tmp.end(), b->begin(), b->end());
        }
        gs = &gs_tmp; gz = &gz_tmp;
    }
    int up_lin(const HostWeights &hw, const std::string &name, int N, int K, WMat *out) {
        const std::vector<float> *gs, *gz;
        grid_of(hw, {name}, gs, gz);
        return up_mat(hw.get(name), N, K, out, gs, gz);
    }

    // encoder layer i (everything but its linear_pos, which prepare_pos stacks with the other layers')
    int prepare_layer(const HostWeights &hw, int i) {
        std::string p = "encoder.layers." + std::to_string(i) + ".";
        LayerW &L = mw.L[i];
        const char *lns[5] = {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"};
        for (int k = 0; k < 5; ++k) {
            TRY(up(hw.get(p + lns[k] + ".weight"), &L.ln_g[k]));
            TRY(up(hw.get(p + lns[k] + ".bias"), &L.ln_b[k]));
        }
        TRY(up_lin(hw, p + "feed_forward1.linear1.weight", QV_FF, QV_D, &L.ff1_w1));
        TRY(up(hw.get(p + "feed_forward1.linear1.bias"), &L.ff1_b1));
        TRY(up_lin(hw, p + "feed_forward1.linear2.weight", QV_D, QV_FF, &L.ff1_w2));
        TRY(up(hw.get(p + "feed_forward1.linear2.bias"), &L.ff1_b2));
        TRY(up_lin(hw, p + "feed_forward2.linear1.weight", QV_FF, QV_D, &L.ff2_w1));
        TRY(up(hw.get(p + "feed_forward2.linear1.bias"), &L.ff2_b1));
        TRY(up_lin(hw, p + "feed_forward2.linear2.weight", QV_D, QV_FF, &L.ff2_w2));
        TRY(up(hw.get(p + "feed_forward2.linear2.bias"), &L.ff2_b2));
        {
            std::vector<float> w, b;
            for (const char *lin : {"linear_q", "linear_k", "linear_v"}) {
                const auto &ww = hw.get(p + "self_attn." + lin + ".weight");
                const auto &bb = hw.get(p + "self_attn." + lin + ".bias");
                w.insert(w.end(), ww.begin(), ww.end());
                b.insert(b.end(), bb.begin(), bb.end());
            }
            const std::vector<float> *gs, *gz;
            grid_of(hw, {p + "self_attn.linear_q.weight", p + "self_attn.linear_k.weight", p + "self_attn.linear_v.weight"}, gs, gz);
            TRY(up_mat(w, 3 * QV_D, QV_D, &L.qkv_w, gs, gz));
            TRY(up(b, &L.qkv_b));
        }
        TRY(up_lin(hw, p + "self_attn.linear_out.weight", QV_D, QV_D, &L.out_w));
        TRY(up(hw.get(p + "self_attn.linear_out.bias"), &L.out_b));
        TRY(up(hw.get(p + "self_attn.pos_bias_u"), &L.bias_u));
        TRY(up(hw.get(p + "self_attn.pos_bias_v"), &L.bias_v));
        {
            // GLU pairing: 64-column groups = [32 value channels | their 32 gate channels]
            const auto &w = hw.get(p + "conv.pointwise_conv1.weight");
            const auto &b = hw.get(p + "conv.pointwise_conv1.bias");
            std::vector<float> pwm((size_t)2 * QV_D * QV_D);
            std::vector<float> pb(2 * QV_D);
            for (int g = 0; g < QV_D / 32; ++g)
                for (int j = 0; j < 32; ++j) {
                    int ra = g * 32 + j, rg = QV_D + g * 32 + j;
                    int da = g * 64 + j, dg = g * 64 + 32 + j;
                    for (int k = 0; k < QV_D; ++k) {
                        pwm[(size_t)da * QV_D + k] = w[(size_t)ra * QV_D + k];
                        pwm[(size_t)dg * QV_D + k] = w[(size_t)rg * QV_D + k];
                    }
                    pb[da] = b[ra];
                    pb[dg] = b[rg];
                }
            TRY(up_mat8(pwm, 2 * QV_D, QV_D, &L.pw1_w));
            TRY(up(pb, &L.pw1_b));
            // (one scale per tensor: the row permutation changes neither the scale nor the codes)
            if (ort) TRY(up_ort_conv(pwm, 2 * QV_D, 2 * QV_D, QV_D, &L.o_pw1, hw.int8_scale(p + "conv.pointwise_conv1.weight")));
        }
        {
            // fold eval-mode BatchNorm into the depthwise conv
            const auto &w = hw.get(p + "conv.depthwise_conv.weight");
            const auto &b = hw.get(p + "conv.depthwise_conv.bias");
            const auto &g = hw.get(p + "conv.batch_norm.weight");
            const auto &be = hw.get(p + "conv.batch_norm.bias");
            const auto &mu = hw.get(p + "conv.batch_norm.running_mean");
            const auto &var = hw.get(p + "conv.batch_norm.running_var");
            std::vector<float> fw((size_t)QV_D * 9), fb(QV_D);
            for (int c = 0; c < QV_D; ++c) {
                float s = g[c] / sqrtf(var[c] + 1e-5f);
                for (int k = 0; k < 9; ++k) fw[(size_t)c * 9 + k] = w[(size_t)c * 9 + k] * s;
                fb[c] = (b[c] - mu[c]) * s + be[c];
            }
            TRY(up(tap_major(fw, QV_D), &L.dw_w));
            TRY(up(fb, &L.dw_b));
            if (ort) {
                // the reference quantises the RAW depthwise weight; BatchNorm stays a float op behind it
                std::vector<float> al(QV_D), bt(QV_D);
                for (int c = 0; c < QV_D; ++c) {
                    al[c] = g[c] * (1.0f / sqrtf(var[c] + 1e-5f));
                    bt[c] = fmaf(-mu[c], al[c], be[c]);
                }
                TRY(up_ort_dw(w, QV_D, &L.o_dw, hw.int8_scale(p + "conv.depthwise_conv.weight")));
                TRY(up(b, &L.o_dw_b));
                TRY(up(al, &L.bn_alpha));
                TRY(up(bt, &L.bn_beta));
            }
        }
        TRY(up_mat8(hw.get(p + "conv.pointwise_conv2.weight"), QV_D, QV_D, &L.pw2_w));
        if (ort)
            TRY(up_ort_conv(hw.get(p + "conv.pointwise_conv2.weight"), QV_D, QV_D, QV_D, &L.o_pw2,
                            hw.int8_scale(p + "conv.pointwise_conv2.weight")));
        TRY(up(hw.get(p + "conv.pointwise_conv2.bias"), &L.pw2_b));
        return QV_OK;
    }

    // linear_pos of all layers stacked along N into one [17 * 512][512] matrix (one GEMM projects the positions for every
    // layer); a pre-quantised file's grids are stacked alike and used only if every layer has one
    int prepare_pos(const HostWeights &hw) {
        std::vector<float> posw((size_t)N_LAYERS * QV_D * QV_D);
        std::vector<float> pos_gs, pos_gz;
        bool pos_grid = prequant;
        for (int i = 0; i < N_LAYERS; ++i) {
            std::string p = "encoder.layers." + std::to_string(i) + ".";
            const auto &pw = hw.get(p + "self_attn.linear_pos.weight");
            for (size_t k = 0; k < pw.size(); ++k) posw[(size_t)i * QV_D * QV_D + k] = pw[k];
            const std::vector<float> *a = hw.int4_scale(p + "self_attn.linear_pos.weight"), *b = hw.int4_zp(p + "self_attn.linear_pos.weight");
            if (pos_grid && a && b && a->size() == b->size()) {
                pos_gs.insert(pos_gs.end(), a->begin(), a->end());
                pos_gz.insert(pos_gz.end(), b->begin(), b->end());
            } else pos_grid = false;
        }
        TRY(up_mat(posw, N_LAYERS * QV_D, QV_D, &mw.pos_w, pos_grid ? &pos_gs : nullptr, pos_grid ? &pos_gz : nullptr));
        // linear_pos has no bias; the GEMM epilogue always reads one
        TRY(up(std::vector<float>((size_t)N_LAYERS * QV_D, 0.f), &mw.zero_bias));
        return QV_OK;
    }

    int prepare_weights(const HostWeights &hw) {
        TRY(prepare_front(hw));
        for (int i = 0; i < N_LAYERS; ++i) TRY(prepare_layer(hw, i));
        return prepare_pos(hw);
    }
};
