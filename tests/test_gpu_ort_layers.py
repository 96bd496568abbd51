"""Precision 2 (QV_PREC_ORT_MIXED): every one of the 17 encoder layers against the OrtMixed oracle (GPU), the quantisers cut out.

test_gpu_ort_mixed.py checks the conv-module stages at layers 0 / 8 / 16, one whole layer at 5e-2 and everything else through the
log-probs, on clips of 38 / 24 / 14 frames.  Which int8 image, scale, zero-point sum, bias and int4 Linear each launch of each
LAYER reads was held by nothing tighter than the oracle's own reproducibility floor.  Here, on ONE engine:

  * weights: forward_ref.telltale_ort_weights from a weight file -- the telltale set with the three conv weights of each layer
    scaled so that neighbouring layers' int8 scales differ by a third at least;
  * batch: test_gpu_layer_taps.py's, 1 / 33 / 128 / 129 / 257 frames ragged in one call (548 packed rows): both attention
    kernels, utterance boundaries inside GEMM tiles, a one-frame utterance; and once more with the key-tiled kernel everywhere;
  * exact stages, every layer and utterance: tap 3 -> 4 (pointwise_conv1 + GLU) and tap 4 -> 5 (depthwise + BatchNorm + Swish)
    on the device's own tensors, 1e-5 of range;
  * tap 9 -> tap 1: pre_encode.out (and the xscaling) from the device's own conv.6 output;
  * segment A: the device's layer input -> oracle norm_conv output, against tap 3;  segment C: the same input and the device's
    own tap 5 handed over -> oracle layer output, against tap 2 (forward_ref.ort_segments);
  * bound of A, C and pre_encode.out: FLOOR_K x e, e = the envelope of forward_ref.ort_twins() around the oracle on that very
    input, per layer and utterance -- and never above TAP_BOUND = 1.5e-2.  Nothing the device computed enters a bound;
  * power: every planted oracle of layer l (test_forward_ref_host.py: >= 4 bounds from the true one) lies >= 3 bounds from the
    device's tensors of layer l on the 33- and 129-frame rows; a plant inside the cut-out chain >= 99 stage bounds.

Oracle results are computed once per module and never modified."""

import os
import time

import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
FRAMES = [1, 33, 128, 129, 257]
PLANT_ROWS = [1, 3]                  # 33 and 129 frames: the clips test_forward_ref_host.py measures the plants on
SEG_PLANTS = [k for k in FR.PLANTS2 if FR.plant_shows_at_out(k) or FR.plant_shows_at_lnc(k)]
CHAIN_PLANTS = [k for k in FR.PLANTS2 if FR.plant_stage(k)]
_cache = {}
_t0 = time.time()


def _cached(key, make):
    if key not in _cache:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _cache[key] = make()
    return _cache[key]


def _weights():
    return _cached("w", lambda: FR.telltale_ort_weights(R.random_weights(SEED)))


def _batch():
    def make():
        ladder = [FR.samples_for_frames(t) for t in FR.LADDER]
        rows = [FR.LADDER.index(t) for t in FRAMES]
        lens = [ladder[r] for r in rows]
        return FR.clips(ladder, FR.LADDER_AUDIO_SEED)[rows][:, : max(lens)].contiguous(), lens
    return _cached("audio", make)


def _taps_of(eng):
    """x[l] = the input of layer l = the output of layer l - 1; x[0] is tap 1, which the device keeps already scaled by sqrt(512)"""
    shape = (len(FRAMES), max(FRAMES), 512)
    taps = {"x": [eng.forward_tap(1, 0, shape).cpu()] + [eng.forward_tap(2, l, shape).cpu() for l in range(R.N_LAYERS)],
            "c2p": eng.forward_tap(9, 0, (len(FRAMES), max(FRAMES), 10, 256)).cpu()}
    for what, name in ((3, "lnc"), (4, "glu"), (5, "dw")):
        taps[name] = [eng.forward_tap(what, l, shape).cpu() for l in range(R.N_LAYERS)]
    return taps


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """everything the device computes, in one engine's lifetime: the batch with the default kernels and with the key-tiled
    attention kernel at every length (all taps read once each), then each utterance alone"""
    from offline_tarteel_amd.engine import Engine

    path = FR.write_weights(tmp_path_factory.mktemp("ort_layers") / "telltale_ort.qvw", _weights())
    audio, lens = _batch()
    os.environ["QVERSE_DEBUG_TAPS"] = "1"      # read when the engine is created
    try:
        eng = Engine(device=0, with_model=True, weights_path=str(path), precision=2, max_batch=len(lens), max_samples=max(lens))
    finally:
        os.environ.pop("QVERSE_DEBUG_TAPS", None)
    got = {}
    try:
        dev = audio.cuda().contiguous()
        for name, variant in (("default", -1), ("key-tiled", 0)):
            eng.attention_variant(variant)
            try:
                lp, t = eng.forward(dev, lens)
                torch.cuda.synchronize()
                got[name] = {"lp": lp.cpu(), "t": t, "taps": _taps_of(eng)}
            finally:
                eng.attention_variant(-1)
        got["alone"] = []
        for b, n in enumerate(lens):
            lp, t = eng.forward(dev[b: b + 1, :n].contiguous(), [n])
            got["alone"].append((lp.cpu(), t))
    finally:
        eng.close()
    return got


def _cells(name, got):
    """the oracle's segments on the device's tensors of forward `name`: per layer and utterance forward_ref.ort_segments (with the
    plants on the 33- and 129-frame rows of the default forward)"""
    def make():
        w, taps, cells = _weights(), got["taps"], {}
        twins = FR.ort_twins()
        for l in range(R.N_LAYERS):
            for b, n in enumerate(FRAMES):
                plants = SEG_PLANTS if name == "default" and b in PLANT_ROWS else ()
                cells[(l, b)] = FR.ort_segments(w, l, taps["x"][l][b, :n], taps["dw"][l][b, :n], twins, plants,
                                                against=(taps["lnc"][l][b, :n], taps["x"][l + 1][b, :n]))
        return cells
    return _cached(("cells", name), make)


@pytest.fixture(scope="module", params=["default", "key-tiled"])
def run(request, device):
    return {"name": request.param, "got": device[request.param], "cells": _cells(request.param, device[request.param])}


def _stage_check(tag, got, want):
    scale, d = float(want.abs().max()), FR._d(got, want)
    same = float((got == want).float().mean())
    return d, FR.STAGE_REL * scale, f"{tag}: max|d| {d:.3e} of range {scale:.3e}, bit-identical {same:.6f}"


def test_exact_stages_of_every_layer(run):
    """tap 3 -> 4 and tap 4 -> 5 on the device's own tensors, all 17 layers, every utterance: integer arithmetic, 1e-5 of range"""
    w, taps, bad = _weights(), run["got"]["taps"], []
    ops = FR.OrtOps()
    for l in range(R.N_LAYERS):
        for b, n in enumerate(FRAMES):
            for stage, src in (("glu", "lnc"), ("dw", "glu")):
                d, bound, line = _stage_check(f"L{l} {stage}[T={n}]", taps[stage][l][b, :n], FR.ort_stage(w, FR._p(l), stage, taps[src][l][b, :n], ops))
                print(f"[ort-layers] {run['name']} {line}")
                if d > bound:
                    bad.append((l, n, stage, d, bound))
    assert not bad, bad


def test_pre_encode_out_from_the_devices_conv6_output(run):
    """tap 9 -> tap 1 per utterance: the int4 Linear in front of the encoder and the xscaling"""
    w, taps, bad = _weights(), run["got"]["taps"], []
    for b, n in enumerate(FRAMES):
        fl = FR.ort_pre_encode_floor(w, taps["c2p"][b, :n])
        d, bound = FR._d(taps["x"][0][b, :n], fl["ref"]), FR.FLOOR_K * fl["e"]
        print(f"[ort-layers] {run['name']} pre_encode.out T={n}: device vs oracle {d:.3e} <= {bound:.3e} (e {fl['e']:.3e}: {d / fl['e']:.2f} e)")
        assert bound <= FR.TAP_BOUND, (n, bound)
        if d > bound:
            bad.append((n, d, bound))
    assert not bad, bad


def test_segments_a_and_c_of_every_layer(run):
    """device tap 3 against the oracle's lnc (segment A) and device tap 2 against the oracle's layer output with the device's tap 5
    handed over (segment C), both from the device's own layer input: within FLOOR_K x the twins' envelope on that input"""
    taps, bad = run["got"]["taps"], []
    for l in range(R.N_LAYERS):
        for b, n in enumerate(FRAMES):
            seg = run["cells"][(l, b)]
            for name, got, want, e in (("A lnc", taps["lnc"][l][b, :n], seg["lnc"], seg["e_lnc"]), ("C out", taps["x"][l + 1][b, :n], seg["out"], seg["e_out"])):
                d, bound = FR._d(got, want), FR.FLOOR_K * e
                print(f"[ort-layers] {run['name']} layer {l:2d} T={n:3d} {name}: device vs oracle {d:.3e} <= {bound:.3e}  (e {e:.3e}: {d / e:.2f} e)")
                assert 0.0 < bound <= FR.TAP_BOUND, (l, n, name, bound)
                if d > bound:
                    bad.append((l, n, name, f"{d:.3e}", f"{bound:.3e}"))
    assert not bad, bad


def test_a_device_with_a_planted_error_would_miss_its_bound(device):
    """every planted oracle of layer l, evaluated on the device's own input, lies >= 3 bounds from the device's tensor of layer l
    (33- and 129-frame rows): a kernel with that error would sit where the planted oracle sits.  Plants inside the cut-out chain:
    >= 99 stage bounds from the device's stage tensor."""
    w, taps = _weights(), device["default"]["taps"]
    cells = _cells("default", device["default"])
    at_lnc, at_out, at_stage = [], [], []
    for l in range(R.N_LAYERS):
        for b in PLANT_ROWS:
            n, seg = FRAMES[b], cells[(l, b)]
            at_lnc += [(a[0] / (FR.FLOOR_K * seg["e_lnc"]), k, l, n) for k, a in seg["A"].items() if FR.plant_shows_at_lnc(k)]
            at_out += [(a[1] / (FR.FLOOR_K * seg["e_out"]), k, l, n) for k, a in seg["A"].items() if FR.plant_shows_at_out(k)]
            for key in CHAIN_PLANTS:
                stage = FR.plant_stage(key)
                wp, ops = FR.planted2(key, w, l)
                bad = FR.ort_stage(wp, FR._p(l), stage, taps["lnc" if stage == "glu" else "glu"][l][b, :n], ops)
                have = taps[stage][l][b, :n]
                at_stage.append((FR._d(bad, have) / (FR.STAGE_REL * float(have.abs().max())), key, l, n))
    assert len(at_out) == 34 * R.N_LAYERS * 2 and len(at_lnc) == 23 * R.N_LAYERS * 2 and len(at_stage) == 18 * R.N_LAYERS * 2
    for name, rows, least in (("lnc", at_lnc, 3.0), ("layer output", at_out, 3.0), ("stage tensor", at_stage, 99.0)):
        rows.sort()
        for r, key, l, n in rows[:3]:
            print(f"[ort-layers] nearest planted oracle at the {name}: {r:.1f} bounds ({key}, layer {l}, T = {n})")
        low = [(key, l, n, round(r, 2)) for r, key, l, n in rows if r < least]
        assert not low, (name, low)


def test_frame_counts_logprobs_padding_and_batch_invariance(device):
    """the oracle's frame counts, finite normalised posteriors, exact zeros behind each utterance in taps 2 - 5 (the taps are read
    from the packed rows: a wrong row offset shows here), both forwards; each utterance alone == in the batch, bit for bit"""
    for name in ("default", "key-tiled"):
        got = device[name]
        assert got["t"] == FRAMES, name
        for b, n in enumerate(FRAMES):
            lp = got["lp"][b, :n]
            assert bool(torch.isfinite(lp).all()), (name, n)
            assert torch.allclose(lp.exp().sum(-1), torch.ones(n), atol=1e-4), (name, n)
        for key in ("x", "lnc", "glu", "dw"):
            for l, x in enumerate(got["taps"][key]):
                assert tuple(x.shape) == (len(FRAMES), max(FRAMES), 512), (name, key, l)
                for b, n in enumerate(FRAMES):
                    assert bool(torch.isfinite(x[b, :n]).all()), (name, key, l, n)
                    if n < max(FRAMES):
                        assert float(x[b, n:].abs().max()) == 0.0, (name, key, l, n)
    lp = device["default"]["lp"]
    differ = [not torch.equal(device["key-tiled"]["lp"][b, :n], lp[b, :n]) for b, n in enumerate(FRAMES) if 1 < n <= 128]
    assert all(differ), differ                    # another attention kernel did run there
    for b, n in enumerate(FRAMES):
        one, t = device["alone"][b]
        assert t == [n] and torch.equal(one[0, :n], lp[b, :n]), n
    print(f"[ort-layers] module wall time so far {time.time() - _t0:.1f} s (since import)")
