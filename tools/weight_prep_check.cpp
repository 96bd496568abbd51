// dev / test: the weight preparation behind qv_create (csrc/qv_model_prep_host.h) -- host only, no GPU.
//
//     clang++ -std=c++17 -fsanitize=address,undefined tools/weight_prep_check.cpp -o weight_prep_check   (needs _Float16)
//     ./weight_prep_check PRECISION OUT_DIR [--weights weights.bin] [--layers 0,16]
//
// Prepares, through the host sink, the front-end tables, the subsampling and head images, the stacked linear_pos and the
// encoder layers asked for (default: all) from the seeded weights (seed 20260630) or from a weight file, and writes every
// image that exists under PRECISION (0 f16, 1 int4 / int8 weights, 2 the ORT arithmetic) into OUT_DIR as a raw
// little-endian array named after its ModelW member ("c0_w", "o_pw3.wq", "L16.qkv_w.sc", a scale as one float32).
// Exit status 0 and a summary on stdout, 3 and "refused (rc N): message" when the file or its preparation is refused, 2
// for a bad command line.  tests/test_weight_prep_host.py builds and runs it.
typedef _Float16 half_t;
#include "../offline-tarteel_amd/csrc/qv_model_prep_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <string>
#include <vector>

namespace {

struct Dumper {
    const HostSink &sink;
    std::string dir;
    bool ok = true;
    void raw(const std::string &name, const void *data, size_t bytes) {
        std::ofstream f(dir + "/" + name, std::ios::binary);
        f.write((const char *)data, (std::streamsize)bytes);
        if (!f) { fprintf(stderr, "cannot write %s/%s\n", dir.c_str(), name.c_str()); ok = false; }
    }
    void image(const std::string &name, const void *p) {   // (nullptr: no such image under this precision)
        if (!p) return;
        for (const HostSink::Image &im : sink.images)
            if (im.data == p) return raw(name, p, im.bytes);
        fprintf(stderr, "%s: a slot the sink never filled\n", name.c_str());
        ok = false;
    }
    void mat(const std::string &n, const WMat &w) {
        image(n + ".w", w.w); image(n + ".q", w.q); image(n + ".sc", w.sc); image(n + ".q8", w.q8); image(n + ".sc8", w.sc8);
    }
    void conv(const std::string &n, const OrtConv &c) {
        if (!c.wq) return;
        image(n + ".wq", c.wq); image(n + ".wsum", c.wsum); raw(n + ".scale", &c.scale, sizeof(float));
    }
    void dw(const std::string &n, const OrtDw &d) {
        if (!d.wq) return;
        image(n + ".wq", d.wq); raw(n + ".scale", &d.scale, sizeof(float));
    }
};

int refused(int rc, const std::string &err) {
    printf("refused (rc %d): %s\n", rc, err.c_str());
    return 3;
}

int run(int precision, const std::string &out_dir, const char *weights, const std::vector<int> &layers) {
    HostWeights hw;
    std::string err;
    if (weights) {
        if (int rc = load_weight_file(weights, hw, err)) return refused(rc, err);
    } else init_random(hw, 20260630ull);
    HostSink sink;
    ModelW mw = {};
    const bool ort = precision == 2, w4 = precision == 1 || ort;
    WeightPrep<HostSink> prep = {sink, w4, ort, hw.prequantised(), mw, err};
    int rc = prep.build_frontend();
    try {
        if (!rc) rc = prep.prepare_front(hw);
        for (int l : layers)
            if (!rc) rc = prep.prepare_layer(hw, l);
        if (!rc) rc = prep.prepare_pos(hw);
    } catch (const QvMissingWeight &e) {
        return refused(QV_ERR_IO, e.what());
    }
    if (rc) return refused(rc, err);

    Dumper d = {sink, out_dir};
#define IMG(member) d.image(#member, mw.member);
    IMG(window) IMG(twiddle) IMG(mel_lo) IMG(mel_cnt) IMG(mel_w)
    IMG(c0_w) IMG(c0_b) IMG(dw2_w) IMG(dw2_b) IMG(dw5_w) IMG(dw5_b) IMG(pw3_b) IMG(pw6_b) IMG(sub_out_b) IMG(head_b)
    IMG(pw3_w) IMG(pw6_w) IMG(sub_out_w) IMG(head_w) IMG(zero_bias)
#undef IMG
    d.mat("pos_w", mw.pos_w);
    d.dw("o_c0", mw.o_c0); d.dw("o_dw2", mw.o_dw2); d.dw("o_dw5", mw.o_dw5);
    d.conv("o_pw3", mw.o_pw3); d.conv("o_pw6", mw.o_pw6); d.conv("o_head", mw.o_head);
    for (int l : layers) {
        const LayerW &L = mw.L[l];
        const std::string p = "L" + std::to_string(l) + ".";
        for (int k = 0; k < 5; ++k) { d.image(p + "ln_g" + std::to_string(k), L.ln_g[k]); d.image(p + "ln_b" + std::to_string(k), L.ln_b[k]); }
#define MAT(member) d.mat(p + #member, L.member);
#define IMG(member) d.image(p + #member, L.member);
        MAT(ff1_w1) MAT(ff1_w2) MAT(ff2_w1) MAT(ff2_w2) MAT(qkv_w) MAT(out_w) MAT(pw1_w) MAT(pw2_w)
        IMG(ff1_b1) IMG(ff1_b2) IMG(ff2_b1) IMG(ff2_b2) IMG(qkv_b) IMG(out_b) IMG(pw1_b) IMG(pw2_b)
        IMG(bias_u) IMG(bias_v) IMG(dw_w) IMG(dw_b) IMG(o_dw_b) IMG(bn_alpha) IMG(bn_beta)
#undef MAT
#undef IMG
        d.conv(p + "o_pw1", L.o_pw1); d.conv(p + "o_pw2", L.o_pw2); d.dw(p + "o_dw", L.o_dw);
    }
    if (!d.ok) return 2;
    printf("prep ok: prequantised %d, %d Linear tensors on the file's int4 grid, %d as f16 values, %zu images\n", (int)hw.prequantised(),
           mw.prequant_w4_linears, mw.prequant_f16_linears, sink.images.size());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const char *weights = nullptr;
    std::vector<int> layers;
    bool all_layers = true, bad = argc < 3;
    for (int i = 3; i < argc && !bad; i += 2) {
        const std::string opt = argv[i];
        if (i + 1 >= argc) bad = true;
        else if (opt == "--weights") weights = argv[i + 1];
        else if (opt == "--layers") {
            all_layers = false;
            for (const char *s = argv[i + 1]; *s;) {
                char *end;
                const long l = strtol(s, &end, 10);
                if (end == s || l < 0 || l >= N_LAYERS || (*end && *end != ',')) { bad = true; break; }
                layers.push_back((int)l);
                s = *end ? end + 1 : end;
            }
        } else bad = true;
    }
    const std::string prec = bad ? "" : argv[1];
    if (bad || (prec != "0" && prec != "1" && prec != "2")) {
        fprintf(stderr, "usage: weight_prep_check 0|1|2 <out dir> [--weights <path>] [--layers i,j,...]\n");
        return 2;
    }
    if (all_layers)
        for (int l = 0; l < N_LAYERS; ++l) layers.push_back(l);
    return run(prec[0] - '0', argv[2], weights, layers);
}
