// qv_weights_host.h -- where the acoustic model's weights come from, on the host: the tensors the model needs
// (weight_shapes), the seeded init, the flat weight file.  HIP-free (the standard library only), so
// tools/file_readers_check.cpp runs the file reader under ASan + UBSan on a machine without a GPU; qv_model_prep_host.h
// lays the tensors out for the device.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <fstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "qv_limits.h"

// thrown by HostWeights::get for a tensor the source does not hold; qv_model_create turns it into QV_ERR_IO
struct QvMissingWeight : std::runtime_error {
    explicit QvMissingWeight(const std::string &name) : std::runtime_error("weights lack tensor " + name) {}
};

struct HostWeights {
    std::unordered_map<std::string, std::vector<float>> t;
    // load_weight_file and init_random provide every name of weight_shapes(), so this fails only for a name outside that list
    const std::vector<float> &get(const std::string &n) const {
        auto it = t.find(n);
        if (it == t.end()) throw QvMissingWeight(n);
        return it->second;
    }
    // A file converted from the reference's quantised ONNX (tools/convert_weights.py --onnx) says so with the marker
    // tensor "qv.prequantised": its Linear weights are the dequantised MatMulNBits values (zero points included) and
    // each int8 Conv weight comes with "<key>#int8_scale", the scale onnxruntime stored.  Such weights are never
    // re-quantised: Linear layers run the values as they are (f16), precision 2 puts the Conv weights back on their
    // integers with the FILE's scale.
    bool prequantised() const {
        auto it = t.find("qv.prequantised");
        return it != t.end() && !it->second.empty() && it->second[0] != 0.f;
    }
    // MatMulNBits' own grid of a Linear weight, block 128: "<key>#int4_scale" / "<key>#int4_zp", [N][K/128] each (absent for
    // other block sizes: such a tensor runs as its dequantised f16 values)
    const std::vector<float> *int4_scale(const std::string &n) const { auto it = t.find(n + "#int4_scale"); return it == t.end() ? nullptr : &it->second; }
    const std::vector<float> *int4_zp(const std::string &n) const { auto it = t.find(n + "#int4_zp"); return it == t.end() ? nullptr : &it->second; }
    float int8_scale(const std::string &n) const {   // 0: none given (derive max|w| / 127)
        auto it = t.find(n + "#int8_scale");
        return it != t.end() && it->second.size() == 1 ? it->second[0] : 0.f;
    }
};

struct Shape { std::string name; std::vector<int> dims; };

inline std::vector<Shape> weight_shapes() {
    std::vector<Shape> s;
    auto add = [&](const std::string &n, std::vector<int> d) { s.push_back({n, d}); };
    const char *pe = "encoder.pre_encode.";
    add(std::string(pe) + "conv.0.weight", {QV_SUBC, 1, 3, 3}); add(std::string(pe) + "conv.0.bias", {QV_SUBC});
    add(std::string(pe) + "conv.2.weight", {QV_SUBC, 1, 3, 3}); add(std::string(pe) + "conv.2.bias", {QV_SUBC});
    add(std::string(pe) + "conv.3.weight", {QV_SUBC, QV_SUBC, 1, 1}); add(std::string(pe) + "conv.3.bias", {QV_SUBC});
    add(std::string(pe) + "conv.5.weight", {QV_SUBC, 1, 3, 3}); add(std::string(pe) + "conv.5.bias", {QV_SUBC});
    add(std::string(pe) + "conv.6.weight", {QV_SUBC, QV_SUBC, 1, 1}); add(std::string(pe) + "conv.6.bias", {QV_SUBC});
    add(std::string(pe) + "out.weight", {QV_D, QV_SUBC * 10}); add(std::string(pe) + "out.bias", {QV_D});
    add("ctc_decoder.decoder_layers.0.weight", {QV_VOCAB, QV_D, 1}); add("ctc_decoder.decoder_layers.0.bias", {QV_VOCAB});
    for (int i = 0; i < QV_N_LAYERS; ++i) {
        std::string p = "encoder.layers." + std::to_string(i) + ".";
        for (const char *ln : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) {
            add(p + ln + ".weight", {QV_D}); add(p + ln + ".bias", {QV_D});
        }
        for (const char *ff : {"feed_forward1", "feed_forward2"}) {
            add(p + ff + ".linear1.weight", {QV_FF, QV_D}); add(p + ff + ".linear1.bias", {QV_FF});
            add(p + ff + ".linear2.weight", {QV_D, QV_FF}); add(p + ff + ".linear2.bias", {QV_D});
        }
        for (const char *lin : {"linear_q", "linear_k", "linear_v", "linear_out"}) {
            add(p + "self_attn." + lin + ".weight", {QV_D, QV_D}); add(p + "self_attn." + lin + ".bias", {QV_D});
        }
        add(p + "self_attn.linear_pos.weight", {QV_D, QV_D});
        add(p + "self_attn.pos_bias_u", {QV_H, QV_DK}); add(p + "self_attn.pos_bias_v", {QV_H, QV_DK});
        add(p + "conv.pointwise_conv1.weight", {2 * QV_D, QV_D, 1}); add(p + "conv.pointwise_conv1.bias", {2 * QV_D});
        add(p + "conv.depthwise_conv.weight", {QV_D, 1, 9}); add(p + "conv.depthwise_conv.bias", {QV_D});
        add(p + "conv.batch_norm.weight", {QV_D}); add(p + "conv.batch_norm.bias", {QV_D});
        add(p + "conv.batch_norm.running_mean", {QV_D}); add(p + "conv.batch_norm.running_var", {QV_D});
        add(p + "conv.pointwise_conv2.weight", {QV_D, QV_D, 1}); add(p + "conv.pointwise_conv2.bias", {QV_D});
    }
    return s;
}

inline bool ends_with(const std::string &s, const char *suf) {
    size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// seeded init: integer hash -> Irwin-Hall(4 bytes) -> affine; exact in f32 and mirrored by
// oracle/fastconformer_ref.py::random_weights
inline void random_tensor(const Shape &sh, uint64_t seed, std::vector<float> &v) {
    size_t n = 1;
    for (int d : sh.dims) n *= (size_t)d;
    uint64_t h = 0xCBF29CE484222325ull;
    for (unsigned char c : sh.name) h = (h ^ c) * 0x100000001B3ull;
    uint64_t key = h ^ (seed * 0x9E3779B97F4A7C15ull);
    float off = 0.f, sc = 0.f;
    bool ab = false;
    const std::string &nm = sh.name;
    if (ends_with(nm, "running_var")) { off = 1.f; sc = 0.1f; ab = true; }
    else if (ends_with(nm, "running_mean")) { off = 0.f; sc = 0.1f; }
    else if (nm.find(".norm_") != std::string::npos || nm.find("batch_norm") != std::string::npos) {
        if (ends_with(nm, "weight")) { off = 1.f; sc = 0.1f; } else { off = 0.f; sc = 0.1f; }
    } else if (ends_with(nm, "bias") || nm.find("pos_bias") != std::string::npos) { off = 0.f; sc = 0.1f; }
    else { size_t fan_in = n / (size_t)sh.dims[0]; sc = 1.0f / sqrtf((float)fan_in); }
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t x = (uint64_t)i + key + 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        int s4 = (int)(z & 0xFF) + (int)((z >> 8) & 0xFF) + (int)((z >> 16) & 0xFF) + (int)((z >> 24) & 0xFF) - 510;
        float zn = (float)s4 * (1.0f / 147.8f);
        if (ab) zn = fabsf(zn);
        float prod = sc * zn;
        v[i] = off + prod;
    }
}

inline void init_random(HostWeights &hw, uint64_t seed) {
    for (const Shape &sh : weight_shapes()) {
        std::vector<float> v;
        random_tensor(sh, seed, v);
        hw.t[sh.name] = std::move(v);
    }
}

// flat weight file: "QVWT0001", u32 count, then per tensor {u32 name_len, name, u32 numel, f32 data}.  The counts in
// the file are held against the bytes that are left before anything is allocated from them.
inline int load_weight_file(const char *path, HostWeights &hw, std::string &err) {
    auto fail = [&](const std::string &msg) { err = msg; return (int)QV_ERR_IO; };
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return fail(std::string("No weight file at ") + path);
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    char magic[8];
    uint32_t cnt = 0;
    f.read(magic, 8);
    f.read((char *)&cnt, 4);
    if (!f || memcmp(magic, "QVWT0001", 8)) return fail("weight file malformed (bad magic)");
    uint64_t left = size - 12;   // bytes behind the read position
    if (cnt > left / 8) return fail("weight file malformed (" + std::to_string(cnt) + " tensors do not fit its " + std::to_string(size) + " bytes)");
    for (uint32_t i = 0; i < cnt; ++i) {
        uint32_t nl = 0, ne = 0;
        if (left < 4) return fail("weight file truncated");
        f.read((char *)&nl, 4);
        left -= 4;
        if (!f || nl > 512 || (uint64_t)nl + 4 > left) return fail("weight file malformed");
        std::string name(nl, '\0');
        f.read(&name[0], nl);
        f.read((char *)&ne, 4);
        left -= (uint64_t)nl + 4;
        if (!f || (uint64_t)ne * 4 > left) return fail("weight file truncated");
        std::vector<float> v(ne);
        f.read((char *)v.data(), (std::streamsize)ne * 4);
        left -= (uint64_t)ne * 4;
        if (!f) return fail("weight file truncated");
        hw.t[name] = std::move(v);
    }
    for (const Shape &sh : weight_shapes()) {
        size_t n = 1;
        for (int d : sh.dims) n *= (size_t)d;
        auto it = hw.t.find(sh.name);
        if (it == hw.t.end() || it->second.size() != n) return fail("weight file lacks tensor or wrong size: " + sh.name);
    }
    return QV_OK;
}
