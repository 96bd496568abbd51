"""The weight preparation behind qv_create (csrc/qv_model_prep_host.h: the named tensors of a weight source -> every image
the kernels read) is pure host logic.  tools/weight_prep_check.cpp is built here with a host compiler that has _Float16,
under AddressSanitizer + UBSan, and run as a plain executable: it prepares the front end, the subsampling and head images,
the stacked linear_pos and the first and the last encoder layer through the host sink, and every image it writes must
equal a numpy restatement of the layout (drawing on oracle/fastconformer_ref.py for the weights and the quantisers) --
for the three precisions from the seeded weights, and for a pre-quantised file written here."""
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import fastconformer_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"
SEED = 20260630
LAYERS = (0, R.N_LAYERS - 1)
REFUSED, QV_ERR_IO = 3, 2
HEAD_N = 1152
D, FF, SUBC = R.D_MODEL, R.FF, R.SUB_CH
f16, f32, f64 = np.float16, np.float32, np.float64
PE, HEAD = "encoder.pre_encode.", "ctc_decoder.decoder_layers.0."
LINEARS = {"ff1_w1": "feed_forward1.linear1", "ff1_w2": "feed_forward1.linear2", "ff2_w1": "feed_forward2.linear1",
           "ff2_w2": "feed_forward2.linear2", "out_w": "self_attn.linear_out"}
QKV = ("self_attn.linear_q", "self_attn.linear_k", "self_attn.linear_v")


def layer(i):
    return f"encoder.layers.{i}."


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    src = ROOT / "tools" / "weight_prep_check.cpp"
    headers = [CSRC / h for h in ("qv_model_prep_host.h", "qv_weights_host.h", "qv_wpack_host.h", "qv_limits.h")]
    for f in (src, *headers):   # no HIP behind them
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    prep_includes = set(re.findall(r'#include\s*"([^"]+)"', headers[0].read_text()))
    assert prep_includes == {"qv_limits.h", "qv_weights_host.h", "qv_wpack_host.h"}, prep_includes
    # half_t is _Float16: g++ before 13 does not have it, clang++ (ROCm's, as a plain host compiler) does
    tmp = tmp_path_factory.mktemp("weight_prep")
    (tmp / "probe.cpp").write_text("int main() { _Float16 h = (_Float16)1.5f; return (float)h == 1.5f ? 0 : 1; }\n")
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    names = [os.environ.get("CXX", "c++"), "clang++", str(rocm / "lib/llvm/bin/clang++"), str(rocm / "llvm/bin/clang++"), "g++"]
    cxx = next((c for c in filter(None, map(shutil.which, names))
                if subprocess.run([c, "-std=c++17", str(tmp / "probe.cpp"), "-o", str(tmp / "probe")], capture_output=True, timeout=120).returncode == 0), None)
    assert cxx, "no host C++ compiler with _Float16"
    exe = tmp / "weight_prep_check"
    # the sanitizer runtimes are linked INTO the executable; -ffp-contract=off as in the library's own build
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static_rt, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
        return p

    return run


# ---------------------------------------------------------------- the weights ----
def seeded(name):
    """one tensor of R.random_weights(SEED), without making the other 550"""
    shape = R.weight_shapes()[name]
    z = R._noise(int(np.prod(shape)), (R._fnv1a(name) ^ (SEED * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF)
    off, sc, ab = R.init_rule(name, shape)
    return (f32(off) + f32(sc) * (np.abs(z) if ab else z)).astype(f32).reshape(shape)


def prepared_names():
    return [n for n in R.weight_shapes() if n.startswith((PE, HEAD, *map(layer, LAYERS))) or n.endswith("linear_pos.weight")]


@pytest.fixture(scope="module")
def seeded_weights():
    w = {n: seeded(n) for n in prepared_names()}
    full = R.random_weights(SEED, n_layers=1)   # the mirror itself, where it is cheap: layer 0 and everything outside the layers
    assert all(np.array_equal(w[n], t.numpy()) for n, t in full.items())
    return w


# ---------------------------------------------------------------- numpy restatements of the layouts ----
def same(got, want, what):
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, got.size, want.dtype, want.size)
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), what   # bit for bit: -0.0 is not 0.0 here


def within_one_ulp(got, want64, what):
    """float32 `got` against a float64 value: at most one float32 ulp apart"""
    assert got.dtype == f32 and got.shape == want64.shape, what
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want64.astype(f32)))).astype(f64)
    assert np.all(np.abs(got.astype(f64) - want64) <= ulp), what


def tap_major(w, C):
    return w.reshape(C, 9).T   # [C][9] -> [9][C]


def glu_paired(w):
    """rows of pointwise_conv1 in 64-row groups: 32 value channels, then their 32 gate channels"""
    a, g = w[:D].reshape(D // 32, 32, -1), w[D:].reshape(D // 32, 32, -1)
    return np.concatenate([a, g], axis=1).reshape(w.shape)


def int4_own(w):
    """qv_pack_w4's codes, block scales and zero points for w [N][K] (the arithmetic of R.quant_dequant_int4)"""
    N, K = w.shape
    wb = w.reshape(N, K // 128, 128)
    vmax = np.take_along_axis(wb, np.abs(wb).argmax(-1)[..., None], -1)[..., 0]
    scale = (vmax / f32(-8.0)).astype(f32)
    with np.errstate(divide="ignore"):
        rs = np.where(scale != 0, f32(1.0) / scale, f32(0.0)).astype(f32)
    q = np.clip(np.floor((wb * rs[..., None]).astype(f32) + f32(8.0) + f32(0.5)), 0, 15).astype(f32)
    assert np.array_equal(((q - f32(8.0)) * scale.astype(f16).astype(f32)[..., None]).reshape(N, K), R.quant_dequant_int4(w))
    return q.reshape(N, K).astype(np.uint8), scale, np.full_like(scale, 8.0)


def int4_given(w, scale, zp):
    """qv_pack_w4_given's codes: rint(w / scale + zp) in float32"""
    N, K = w.shape
    t = (w.reshape(N, K // 128, 128) / scale[..., None]).astype(f32) + zp[..., None]
    q = np.rint(t)
    assert np.all(np.abs(t - q) <= 1e-3) and q.min() >= 0 and q.max() <= 15
    return q.reshape(N, K).astype(np.uint8)


def w4_image(q, scale, zp):
    """the W4A16 image of codes q [N][K]: 64 x 64 tiles of nibbles, 2 KB each, [N/64][K/64][64 rows][32 B]; inside a row the
    4-byte chunk c of 8 codes sits at c ^ ((n >> 2) & 7), code k = 2p in nibble p and k = 2p + 1 in nibble p + 4 of its chunk
    (qv_w4_put).  The scale table is [K/128][N] pairs {half(scale), half(1024 + zp)}."""
    N, K = q.shape
    n, kk = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    kt, c, e = kk >> 6, (kk & 63) >> 3, kk & 7
    nib = (e >> 1) + 4 * (e & 1)
    byte = ((n >> 6) * (K // 64) + kt) * 2048 + (n & 63) * 32 + (c ^ ((n >> 2) & 7)) * 4 + (nib >> 1)
    out = np.zeros(N * K // 2, np.uint8)
    lo, hi = (nib & 1) == 0, (nib & 1) == 1
    out[byte[lo]] = q[lo]
    out[byte[hi]] |= q[hi] << 4
    tab = np.stack([scale.T.astype(f16), (f32(1024.0) + zp.T).astype(f16)], axis=-1)
    return out, tab.ravel()


def w8_image(w):
    """qv_pack_w8: per-row symmetric int8 (R.quant_dequant_int8), q + 128 in [N/64][K/64][64 rows][64 B] with the 8-byte chunk
    c of a row at c ^ ((n >> 2) & 7)"""
    N, K = w.shape
    amax = np.abs(w).max(axis=1, keepdims=True)
    scale = np.where(amax > 0, amax / f32(127.0), f32(1.0)).astype(f32)
    q = np.clip(np.floor((w / scale).astype(f32) + f32(0.5)), -127, 127)
    assert np.array_equal((q * scale).astype(f32), R.quant_dequant_int8(w))
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    byte = ((n >> 6) * (K // 64) + (k >> 6)) * 4096 + (n & 63) * 64 + ((((k & 63) >> 3) ^ ((n >> 2) & 7)) << 3) + (k & 7)
    out = np.zeros(N * K, np.uint8)
    out[byte] = (q + 128).astype(np.uint8)
    return out, scale.ravel()


def ort_codes(w, given=None):
    """quantize_dynamic(QInt8)'s per-tensor codes and scale (R.quantize_weight_int8), or the codes under a GIVEN scale"""
    if given is None:
        q, sw = R.quantize_weight_int8(torch.from_numpy(w))
        return q.numpy().astype(np.int8), f32(sw)
    return np.clip(np.rint((w / f32(given)).astype(f32)), -127, 127).astype(np.int8), f32(given)


def frontend_tables():
    """window, twiddles and the Slaney filterbank in float64 (R.mel_filterbank's recipe, unrounded)"""
    win = np.zeros(512)
    win[56:456] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 399.0)
    ang = -2.0 * np.pi * np.arange(256) / 512.0
    tw = np.stack([np.cos(ang), np.sin(ang)], axis=-1).ravel()
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    hz_to_mel = lambda f: min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp   # noqa: E731
    mlo, mhi = hz_to_mel(0.0), hz_to_mel(8000.0)
    m = mlo + (mhi - mlo) * np.arange(R.N_MELS + 2) / (R.N_MELS + 1)
    mel_f = np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)
    fk = 8000.0 * np.arange(257) / 256.0
    fb = np.zeros((R.N_MELS, 257))
    for i in range(R.N_MELS):
        lower = (fk - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fk) / (mel_f[i + 2] - mel_f[i + 1])
        fb[i] = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[i + 2] - mel_f[i]))
    assert np.allclose(fb, R.mel_filterbank(), rtol=1e-6, atol=1e-12)
    return win, tw, fb


class Dump:
    """the images one run wrote; every file has to be asked for exactly once"""

    def __init__(self, d):
        self.d, self.left = Path(d), {p.name for p in Path(d).iterdir()}

    def get(self, name, dtype):
        assert name in self.left, f"{name}: not written (or checked twice)"
        self.left.remove(name)
        return np.fromfile(self.d / name, dtype)

    def absent(self, *names):
        assert not self.left.intersection(names), self.left.intersection(names)


def check_frontend(dump):
    win, tw, fb = frontend_tables()
    within_one_ulp(dump.get("window", f32), win, "window")
    within_one_ulp(dump.get("twiddle", f32), tw, "twiddle")
    nz = [np.flatnonzero(fb[i].astype(f32) > 0) for i in range(R.N_MELS)]
    lo, cnt = np.array([k[0] for k in nz], np.int32), np.array([k[-1] - k[0] + 1 for k in nz], np.int32)
    assert cnt.max() <= 32
    same(dump.get("mel_lo", np.int32), lo, "mel_lo")
    same(dump.get("mel_cnt", np.int32), cnt, "mel_cnt")
    got = dump.get("mel_w", f32).reshape(32, R.N_MELS)
    want = np.zeros((32, R.N_MELS))
    tap = np.arange(32)[:, None] < cnt[None, :]   # tap k of filter m at [k][m]
    for m in range(R.N_MELS):
        want[:cnt[m], m] = fb[m, lo[m]:lo[m] + cnt[m]]
    within_one_ulp(got, want, "mel_w")
    assert np.all(got[~tap] == 0.0), "weights outside a filter's cnt taps"
    # placement: a filter's first and last tap are where lo and cnt say, and nonzero by their definition
    assert np.all(got[0] > 0) and np.all(got[cnt - 1, np.arange(R.N_MELS)] > 0)
    assert np.array_equal(got > 0, (want.astype(f32) > 0)), "tap-major placement"


def check_linear(dump, img, w, mode, grid=None):
    """a Linear weight image: "f16" values, the engine's "own" int4 grid, or the file's `grid` (scale, zp)"""
    if mode == "f16":
        same(dump.get(img + ".w", f16), w.astype(f16), img)
    else:
        q, scale, zp = int4_own(w) if mode == "own" else (int4_given(w, *grid), *grid)
        nib, tab = w4_image(q, scale, zp)
        same(dump.get(img + ".q", np.uint8), nib, img + ".q")
        same(dump.get(img + ".sc", f16), tab, img + ".sc")
    dump.absent(img + ".w", img + ".q", img + ".sc", img + ".q8", img + ".sc8")


def check_pointwise(dump, img, w, prec, prequant):
    """a pointwise-conv weight of the encoder: f16, per-channel int8 under precision 1, nothing under ORT (o_pw* holds it)"""
    if prec == 1 and not prequant:
        q8, sc8 = w8_image(w)
        same(dump.get(img + ".q8", np.uint8), q8, img + ".q8")
        same(dump.get(img + ".sc8", f32), sc8, img + ".sc8")
    elif prec != 2:
        same(dump.get(img + ".w", f16), w.astype(f16), img)
    dump.absent(img + ".w", img + ".q", img + ".sc", img + ".q8", img + ".sc8")


def check_ort_conv(dump, img, w, n_rows, given):
    q, sw = ort_codes(w, given)
    padded = np.zeros((n_rows, w.shape[1]), np.int8)
    padded[:w.shape[0]] = q
    same(dump.get(img + ".wq", np.int8), padded, img + ".wq")
    same(dump.get(img + ".wsum", np.int32), padded.astype(np.int32).sum(axis=1, dtype=np.int32), img + ".wsum")
    same(dump.get(img + ".scale", f32), np.array([sw], f32), img + ".scale")
    return q


def check_ort_dw(dump, img, w, C, given):
    q, sw = ort_codes(w.reshape(C, 9), given)
    same(dump.get(img + ".wq", f32), tap_major(q.astype(f32), C), img + ".wq")
    same(dump.get(img + ".scale", f32), np.array([sw], f32), img + ".scale")
    return q


def check_run(d, W, prec, prequant=False, lin=None, given=None, layers=LAYERS):
    """every image of one run.  lin: {image: ("f16" | "own" | "grid", grid)} for the Linear weights (default: the precision's
    own form); given: {tensor: the int8 scale the file stores}.  Returns the ORT codes by tensor name."""
    dump, lin, given, codes = Dump(d), lin or {}, given or {}, {}
    own = ("own" if prec else "f16", None)
    ort = prec == 2
    check_frontend(dump)
    # ---- subsampling and head
    for img, conv in (("c0", "conv.0"), ("dw2", "conv.2"), ("dw5", "conv.5")):
        same(dump.get(img + "_w", f32), tap_major(W[PE + conv + ".weight"], SUBC), img + "_w")
        same(dump.get(img + "_b", f32), W[PE + conv + ".bias"], img + "_b")
        if ort:
            n = PE + conv + ".weight"
            codes[n] = check_ort_dw(dump, "o_" + img, W[n], SUBC, given.get(n))
    for img, conv in (("pw3", "conv.3"), ("pw6", "conv.6")):
        w = W[PE + conv + ".weight"].reshape(SUBC, SUBC)
        same(dump.get(img + "_w", f16), w.astype(f16), img + "_w")
        same(dump.get(img + "_b", f32), W[PE + conv + ".bias"], img + "_b")
        if ort:
            n = PE + conv + ".weight"
            codes[n] = check_ort_conv(dump, "o_" + img, w, SUBC, given.get(n))
    w = W[PE + "out.weight"]
    if ort and not prequant:   # quantised along the ORIGINAL K order, then run as f16 values
        w = R.quant_dequant_int4_f32scale(w)
    same(dump.get("sub_out_w", f16), w.reshape(D, SUBC, 10).transpose(0, 2, 1).astype(f16), "sub_out_w")   # c*10+f -> f*256+c
    same(dump.get("sub_out_b", f32), W[PE + "out.bias"], "sub_out_b")
    hw = W[HEAD + "weight"].reshape(R.VOCAB, D)
    same(dump.get("head_w", f16), np.concatenate([hw, np.zeros((HEAD_N - R.VOCAB, D), f32)]).astype(f16), "head_w")
    same(dump.get("head_b", f32), np.concatenate([W[HEAD + "bias"], np.zeros(HEAD_N - R.VOCAB, f32)]), "head_b")
    if ort:
        codes[HEAD + "weight"] = check_ort_conv(dump, "o_head", hw, HEAD_N, given.get(HEAD + "weight"))
    # ---- linear_pos of all layers stacked along N
    check_linear(dump, "pos_w", np.concatenate([W[layer(i) + "self_attn.linear_pos.weight"] for i in range(R.N_LAYERS)]), *lin.get("pos_w", own))
    same(dump.get("zero_bias", f32), np.zeros(R.N_LAYERS * D, f32), "zero_bias")
    # ---- encoder layers
    for l in layers:
        p, L = layer(l), f"L{l}."
        for k, ln in enumerate(("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out")):
            same(dump.get(f"{L}ln_g{k}", f32), W[p + ln + ".weight"], ln)
            same(dump.get(f"{L}ln_b{k}", f32), W[p + ln + ".bias"], ln)
        for img, name in LINEARS.items():
            check_linear(dump, L + img, W[p + name + ".weight"], *lin.get(L + img, own))
        for img, name in (("ff1_b1", "feed_forward1.linear1"), ("ff1_b2", "feed_forward1.linear2"), ("ff2_b1", "feed_forward2.linear1"),
                          ("ff2_b2", "feed_forward2.linear2"), ("out_b", "self_attn.linear_out"), ("pw2_b", "conv.pointwise_conv2")):
            same(dump.get(L + img, f32), W[p + name + ".bias"], L + img)
        check_linear(dump, L + "qkv_w", np.concatenate([W[p + n + ".weight"] for n in QKV]), *lin.get(L + "qkv_w", own))
        same(dump.get(L + "qkv_b", f32), np.concatenate([W[p + n + ".bias"] for n in QKV]), L + "qkv_b")
        same(dump.get(L + "bias_u", f32), W[p + "self_attn.pos_bias_u"], L + "bias_u")
        same(dump.get(L + "bias_v", f32), W[p + "self_attn.pos_bias_v"], L + "bias_v")
        pw1 = glu_paired(W[p + "conv.pointwise_conv1.weight"].reshape(2 * D, D))
        check_pointwise(dump, L + "pw1_w", pw1, prec, prequant)
        same(dump.get(L + "pw1_b", f32), glu_paired(W[p + "conv.pointwise_conv1.bias"]), L + "pw1_b")
        pw2 = W[p + "conv.pointwise_conv2.weight"].reshape(D, D)
        check_pointwise(dump, L + "pw2_w", pw2, prec, prequant)
        # BatchNorm folded into the depthwise conv: pure float32 +, /, sqrt, *
        dw, b = W[p + "conv.depthwise_conv.weight"].reshape(D, 9), W[p + "conv.depthwise_conv.bias"]
        g, be = W[p + "conv.batch_norm.weight"], W[p + "conv.batch_norm.bias"]
        mu, var = W[p + "conv.batch_norm.running_mean"], W[p + "conv.batch_norm.running_var"]
        s = g / np.sqrt(var + f32(1e-5))
        assert s.dtype == f32
        same(dump.get(L + "dw_w", f32), tap_major(dw * s[:, None], D), L + "dw_w")
        same(dump.get(L + "dw_b", f32), (b - mu) * s + be, L + "dw_b")
        if ort:
            n = p + "conv.pointwise_conv1.weight"
            codes[n] = check_ort_conv(dump, L + "o_pw1", pw1, 2 * D, given.get(n))
            n = p + "conv.pointwise_conv2.weight"
            codes[n] = check_ort_conv(dump, L + "o_pw2", pw2, D, given.get(n))
            n = p + "conv.depthwise_conv.weight"
            codes[n] = check_ort_dw(dump, L + "o_dw", dw, D, given.get(n))
            same(dump.get(L + "o_dw_b", f32), b, L + "o_dw_b")
            alpha = g * (f32(1.0) / np.sqrt(var + f32(1e-5)))
            same(dump.get(L + "bn_alpha", f32), alpha, L + "bn_alpha")
            # one fmaf on the device side of this check, two roundings at most on the float64 route
            within_one_ulp(dump.get(L + "bn_beta", f32), -mu.astype(f64) * alpha.astype(f64) + be.astype(f64), L + "bn_beta")
    assert not dump.left, f"images nobody expected under precision {prec}: {sorted(dump.left)}"
    return codes


def summary(p):
    m = re.match(r"prep ok: prequantised (\d), (\d+) Linear tensors on the file's int4 grid, (\d+) as f16 values, (\d+) images", p.stdout)
    assert p.returncode == 0 and m, (p.returncode, p.stdout, p.stderr)
    return tuple(map(int, m.groups()))


# ---------------------------------------------------------------- the seeded weights, three precisions ----
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_seeded_images_are_what_the_layouts_say(checker, seeded_weights, tmp_path, prec):
    p = checker(prec, tmp_path, "--layers", ",".join(map(str, LAYERS)))
    assert summary(p)[:3] == (0, 0, 0), p.stdout
    check_run(tmp_path, seeded_weights, prec)


# ---------------------------------------------------------------- a pre-quantised file ----
def record(name, arr):
    a = np.ascontiguousarray(arr, dtype=f32).ravel()
    return struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", a.size) + a.tobytes()


class WeightFile:
    """a weight file of every tensor of the model (the prepared ones seeded, the others zero), written once; a case appends
    its own tensors behind them -- a later record of a name replaces the earlier one -- and the next case cuts them off"""

    def __init__(self, path, base):
        self.path, self.n = path, 0
        with open(path, "wb") as f:
            f.write(b"QVWT0001" + struct.pack("<I", 0))
            for name, shape in R.weight_shapes().items():
                f.write(record(name, base[name]) if name in base else
                        struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", int(np.prod(shape))))
                if name not in base:
                    f.seek(4 * int(np.prod(shape)), os.SEEK_CUR)   # a hole: zeros
                self.n += 1
            f.truncate(f.tell())
            self.size = f.tell()

    def with_extra(self, extra):
        with open(self.path, "r+b") as f:
            f.truncate(self.size)
            f.seek(self.size)
            for name, arr in extra.items():
                f.write(record(name, arr))
            f.seek(8)
            f.write(struct.pack("<I", self.n + len(extra)))
        return self.path


def on_grid(rng, N, K, symmetric):
    """a Linear weight that sits on an int4 grid of its own: (values, codes, (scale, zero point))"""
    q = rng.integers(0, 16, (N, K))
    scale = (rng.uniform(0.5, 1.5, (N, K // 128)) * 0.01).astype(f32)
    zp = np.full((N, K // 128), 8.0, f32) if symmetric else rng.integers(0, 16, (N, K // 128)).astype(f32)
    w = ((q.reshape(N, K // 128, 128) - zp[..., None]).astype(f32) * scale[..., None]).astype(f32).reshape(N, K)
    return w, q.astype(np.uint8), (scale, zp)


@pytest.fixture(scope="module")
def prequant(seeded_weights, tmp_path_factory):
    """The file, and what it holds.  Grids: layer 0 -- linear1 of FFN 1 has one, linear2 none, linear1 of FFN 2 one of the wrong
    size (block 64), linear2 a scale without zero points, Q/K/V and linear_out have theirs; last layer -- the four FFN Linears
    have theirs (asymmetric), linear_k lacks its own, linear_out has none; linear_pos has one in all 17 layers.  Int8 scales:
    conv.0, conv.3 and layer 0's pointwise_conv1 and depthwise_conv store theirs, the other Conv weights none."""
    rng = np.random.default_rng(SEED)
    W, extra, grids, codes4 = dict(seeded_weights), {"qv.prequantised": [1.0]}, {}, {}
    shapes = R.weight_shapes()

    def gridded(name, symmetric=True, store=("scale", "zp")):
        W[name], codes4[name], grids[name] = on_grid(rng, *shapes[name], symmetric)
        extra[name] = W[name]
        for part, arr in zip(("scale", "zp"), grids[name]):
            if part in store:
                extra[f"{name}#int4_{part}"] = arr

    first, last = layer(LAYERS[0]), layer(LAYERS[1])
    gridded(first + "feed_forward1.linear1.weight")
    gridded(first + "feed_forward2.linear2.weight", store=("scale",))
    extra[first + "feed_forward2.linear1.weight#int4_scale"] = np.ones(FF * D // 64, f32)
    extra[first + "feed_forward2.linear1.weight#int4_zp"] = np.full(FF * D // 64, 8.0, f32)
    for n in (*QKV, "self_attn.linear_out"):
        gridded(first + n + ".weight", symmetric=n != "self_attn.linear_v")
    for n in ("feed_forward1.linear1", "feed_forward1.linear2", "feed_forward2.linear1", "feed_forward2.linear2"):
        gridded(last + n + ".weight", symmetric=False)
    for n in QKV:
        gridded(last + n + ".weight", store=() if n == "self_attn.linear_k" else ("scale", "zp"))
    for i in range(R.N_LAYERS):
        gridded(layer(i) + "self_attn.linear_pos.weight")
    given, codes8 = {}, {}
    for k, name in enumerate((PE + "conv.0.weight", PE + "conv.3.weight", first + "conv.pointwise_conv1.weight", first + "conv.depthwise_conv.weight")):
        given[name] = f32(0.0123 + 0.001 * k)
        codes8[name] = rng.integers(-120, 121, shapes[name]).astype(np.int8)   # (max |q| < 127: a derived scale would differ)
        W[name] = extra[name] = (codes8[name].astype(f32) * given[name]).astype(f32)
        extra[name + "#int8_scale"] = [given[name]]
    file = WeightFile(tmp_path_factory.mktemp("prequant") / "weights.bin", seeded_weights)
    stack = lambda names, part: np.concatenate([grids[n][part] for n in names])   # noqa: E731
    qkv0, pos = [first + n + ".weight" for n in QKV], [layer(i) + "self_attn.linear_pos.weight" for i in range(R.N_LAYERS)]
    grid = lambda n: ("grid", grids[n])   # noqa: E731
    lin = {f"L{LAYERS[0]}.ff1_w1": grid(first + "feed_forward1.linear1.weight"), f"L{LAYERS[0]}.out_w": grid(first + "self_attn.linear_out.weight"),
           f"L{LAYERS[0]}.qkv_w": ("grid", (stack(qkv0, 0), stack(qkv0, 1))), "pos_w": ("grid", (stack(pos, 0), stack(pos, 1)))}
    lin.update({f"L{LAYERS[1]}.{img}": grid(last + LINEARS[img] + ".weight") for img in ("ff1_w1", "ff1_w2", "ff2_w1", "ff2_w2")})
    for img in (f"L{LAYERS[0]}.ff1_w2", f"L{LAYERS[0]}.ff2_w1", f"L{LAYERS[0]}.ff2_w2", f"L{LAYERS[1]}.qkv_w", f"L{LAYERS[1]}.out_w"):
        lin[img] = ("f16", None)
    return {"file": file, "W": W, "extra": extra, "lin": lin, "given": given, "codes4": codes4, "codes8": codes8, "grids": grids}


@pytest.mark.parametrize("prec", [1, 2])
def test_prequantised_file_keeps_its_grids(checker, prequant, tmp_path, prec):
    P = prequant
    p = checker(prec, tmp_path, "--weights", P["file"].with_extra(P["extra"]), "--layers", ",".join(map(str, LAYERS)))
    # on the file's grid: layer 0's linear1, Q/K/V, linear_out; the last layer's four FFN Linears; linear_pos.  As f16 values:
    # layer 0's three Linears without a usable grid; the last layer's Q/K/V (one grid missing: the triple falls back) and linear_out
    assert summary(p)[:3] == (1, 8, 5), p.stdout
    codes = check_run(tmp_path, P["W"], prec, prequant=True, lin=P["lin"], given=P["given"] if prec == 2 else None)
    # the file's integers come back verbatim: the int4 codes of a gridded Linear, the int8 codes under a given scale
    name = layer(LAYERS[0]) + "feed_forward1.linear1.weight"
    assert np.array_equal(int4_given(P["W"][name], *P["grids"][name]), P["codes4"][name])
    if prec == 2:
        for name, q in P["codes8"].items():
            want = glu_paired(q.reshape(2 * D, D)) if name.endswith("pointwise_conv1.weight") else q.reshape(codes[name].shape)
            assert np.array_equal(codes[name], want), name


def test_linear_pos_needs_the_grid_of_every_layer(checker, prequant, tmp_path):
    P = prequant
    extra = {k: v for k, v in P["extra"].items() if k != layer(7) + "self_attn.linear_pos.weight#int4_zp"}
    p = checker(1, tmp_path, "--weights", P["file"].with_extra(extra), "--layers", "")
    assert summary(p)[:3] == (1, 0, 1), p.stdout
    check_run(tmp_path, P["W"], 1, prequant=True, lin={"pos_w": ("f16", None)}, layers=())


def test_weight_off_its_declared_grid_is_refused(checker, prequant, tmp_path):
    P = prequant
    name = layer(LAYERS[0]) + "feed_forward1.linear1.weight"
    w = P["W"][name].copy()
    w[3, 200] += f32(0.3) * P["grids"][name][0][3, 1]   # 0.3 of a step off
    p = checker(1, tmp_path, "--weights", P["file"].with_extra(dict(P["extra"], **{name: w})), "--layers", str(LAYERS[0]))
    assert p.returncode == REFUSED, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.startswith(f"refused (rc {QV_ERR_IO}): pre-quantised weight file: a Linear weight does not sit on the int4 grid it declares"), p.stdout
    assert not list(tmp_path.iterdir())


def test_incomplete_file_is_refused_before_preparation(checker, tmp_path):
    name = b"encoder.pre_encode.conv.0.bias"
    (tmp_path / "w.bin").write_bytes(b"QVWT0001" + struct.pack("<II", 1, len(name)) + name + struct.pack("<I", 3) + bytes(12))
    p = checker(0, tmp_path, "--weights", tmp_path / "w.bin")
    assert p.returncode == REFUSED and p.stdout.startswith(f"refused (rc {QV_ERR_IO}): weight file lacks tensor or wrong size"), p.stdout
