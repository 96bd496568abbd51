"""The tap behind every one of the 17 encoder layers against the fp32 oracle (GPU), on weights where ONE wrong tensor shows.

test_gpu_forward.py taps layers 0 / 3 / 8 / 16 and test_gpu_forward_lengths.py 0 / 8 / 16; the other 13 layers were judged through
the log-probs only, and on the seeded or "sharp" weights a layer that reads a neighbour's bias, LayerNorm or BatchNorm vector, or
its pos_bias_u / v, moves neither by more than the bounds grant.  Here:

  * weights: forward_ref.telltale_weights from a weight file, precision 0 and 1.  On them every per-layer tensor replaced by the
    next layer's (what a pointer or offset slip computes), and seven slips inside a layer (u / v swapped, the two FFN LayerNorms
    or linear2 biases swapped, depthwise taps reversed or one dropped, BatchNorm's mean not scaled), moves that layer's tap by
    >= 4 bounds in every layer -- shown on the CPU by test_forward_ref_host.py with the ORACLE computing the wrong thing;
  * batch: 1 / 33 / 128 / 129 / 257 frames, ragged in one call -- the short-utterance attention kernel and the key-tiled one, a
    partial key tile, a packed row count (548) that is no tile multiple;
  * bounds: tap l <= max(1.5e-2, 1.5 e_tap[l]), e_tap = the reference twins' own distance from fp32 (forward_ref.tap_floor:
    1.5 e_tap stays below 1.5e-2, so it is the project's 1.5e-2); sub <= 5e-2; log-probs by rule (a).

Oracle results are computed once per module and never modified."""

import os

import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R

pytestmark = pytest.mark.gpu

SEED = 7
FRAMES = [1, 33, 128, 129, 257]
PLANT_ROWS = [1, 3]                  # 33 and 129 frames: the clips test_forward_ref_host.py measures the plants on
_cache = {}


def _cached(key, make):
    if key not in _cache:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _cache[key] = make()
    return _cache[key]


def _weights(kind):
    """'telltale', or 'telltale_q' = what a precision-1 engine makes of the telltale file"""
    if kind == "telltale_q":
        return _cached(("w", kind), lambda: R.quantize_linear_weights(_weights("telltale")))
    return _cached(("w", kind), lambda: FR.telltale_weights(R.random_weights(SEED)))


def _batch():
    def make():
        ladder = [FR.samples_for_frames(t) for t in FR.LADDER]
        rows = [FR.LADDER.index(t) for t in FRAMES]
        lens = [ladder[r] for r in rows]
        return FR.clips(ladder, FR.LADDER_AUDIO_SEED)[rows][:, : max(lens)].contiguous(), lens
    return _cached("audio", make)


def _ref(kind):
    """fp32 oracle (log-probs, sub and 17 layer taps), both twins, e, e_tap and the bounds of the whole batch"""
    return _cached(("ref", kind), lambda: FR.tap_floor(_weights(kind), *_batch()))


def _taps_of(eng):
    shape = (len(FRAMES), max(FRAMES), 512)
    return {"sub": eng.forward_tap(1, 0, shape).cpu(), **{f"layer{l}": eng.forward_tap(2, l, shape).cpu() for l in range(R.N_LAYERS)}}


@pytest.fixture(scope="module")
def telltale_file(tmp_path_factory):
    return FR.write_weights(tmp_path_factory.mktemp("layer_taps") / "telltale.qvw", _weights("telltale"))


def _device(p, telltale_file):
    """everything the device computes in precision p, in one engine's lifetime (once per module); the tests only compare"""
    def make():
        from offline_tarteel_amd.engine import Engine

        audio, lens = _batch()
        os.environ["QVERSE_DEBUG_TAPS"] = "1"      # read when the engine is created
        try:
            eng = Engine(device=0, with_model=True, weights_path=str(telltale_file), precision=p, max_batch=len(lens),
                         max_samples=max(lens))
        finally:
            os.environ.pop("QVERSE_DEBUG_TAPS", None)
        try:
            dev = audio.cuda().contiguous()
            lp, t = eng.forward(dev, lens)
            torch.cuda.synchronize()
            got = {"lp": lp.cpu(), "t": t, "taps": _taps_of(eng)}
            if p == 0:
                eng.attention_variant(0)           # the key-tiled kernel at 1 - 128 frames as well
                try:
                    lp0, t0 = eng.forward(dev, lens)
                    torch.cuda.synchronize()
                    got["tiled"] = {"lp": lp0.cpu(), "t": t0, "taps": _taps_of(eng)}
                finally:
                    eng.attention_variant(-1)
        finally:
            eng.close()
        return got
    kind = "telltale_q" if p else "telltale"
    return dict(precision=p, kind=kind, ref=_ref(kind), got=_cached(("device", p), make))


@pytest.fixture(scope="module", params=[0, 1], ids=["precision0", "precision1"])
def run(request, telltale_file):
    return _device(request.param, telltale_file)


def _check_taps(tag, ref, taps):
    """every figure printed, then asserted: per utterance, sub and the 17 layers"""
    T, sub_scale = ref["t"], R.D_MODEL ** 0.5          # the device keeps the xscaled tensor
    rows = [("sub", [FR.maxdiff(taps["sub"][b], ref["taps"]["sub"][b] * sub_scale, n) for b, n in enumerate(T)], FR.SUB_BOUND, ref["e_sub"])]
    for l in range(R.N_LAYERS):
        key = f"layer{l}"
        rows.append((key, [FR.maxdiff(taps[key][b], ref["taps"][key][b], n) for b, n in enumerate(T)], ref["bound_tap"][l], ref["e_tap"][l]))
    for key, d, bound, e in rows:
        print(f"[layer-taps] {tag} {key:8s} T = {' / '.join(map(str, T))}: " + " / ".join(f"{x:.2e}" for x in d)
              + f"   max {max(d):.2e} <= {bound:.2e}   (twins' floor {e:.2e}: {max(d) / e:.2f} e_tap)")
    for key, d, bound, _ in rows:
        for n, x in zip(T, d):
            assert x <= bound, (tag, key, n, x, bound)
    return rows


def _check_padding(tag, taps, T):
    for key, x in taps.items():
        assert tuple(x.shape) == (len(T), max(T), 512), (tag, key, x.shape)
        for b, n in enumerate(T):
            assert bool(torch.isfinite(x[b, :n]).all()), (tag, key, n)
            if n < max(T):
                assert float(x[b, n:].abs().max()) == 0.0, (tag, key, n)


def test_every_layer_tap_against_the_fp32_oracle(run):
    """sub and the taps behind all 17 layers, device vs fp32 oracle, per utterance"""
    assert run["got"]["t"] == run["ref"]["t"] == FRAMES
    _check_taps(f"precision {run['precision']}", run["ref"], run["got"]["taps"])


def test_logprobs_frame_counts_and_padding_rows(run):
    """rule (a) on the log-probs, the oracle's frame counts, normalised posteriors, and exact zeros behind each utterance's last
    frame in every tap (the taps are read from the packed rows: a wrong row offset shows here)"""
    ref, got = run["ref"], run["got"]
    assert got["t"] == ref["t"] == FRAMES
    FR.check_rules(f"layer-taps precision {run['precision']}", got["lp"], ref)
    for b, n in enumerate(FRAMES):
        lp = got["lp"][b, :n]
        assert bool(torch.isfinite(lp).all()), n
        assert torch.allclose(lp.exp().sum(-1), torch.ones(n), atol=1e-4), n
    _check_padding(f"precision {run['precision']}", got["taps"], FRAMES)


def test_every_layer_tap_with_the_key_tiled_kernel_at_every_length(telltale_file):
    """precision 0 again with attention_variant(0): the key-tiled kernel serves the 1-, 33- and 128-frame utterances too"""
    run = _device(0, telltale_file)
    ref, got, tiled = run["ref"], run["got"], run["got"]["tiled"]
    assert tiled["t"] == FRAMES
    differ = [not torch.equal(tiled["lp"][b, :n], got["lp"][b, :n]) for b, n in enumerate(FRAMES) if 1 < n <= 128]
    assert all(differ), differ                    # another kernel did run there (a one-frame softmax is the same in any kernel)
    _check_taps("precision 0, key-tiled kernel", ref, tiled["taps"])
    FR.check_rules("layer-taps precision 0, key-tiled kernel", tiled["lp"], ref)
    _check_padding("precision 0, key-tiled kernel", tiled["taps"], FRAMES)


def test_a_device_with_a_planted_error_would_miss_the_bound(run):
    """The consequence of test_every_plant_shows_at_its_layer_tap (oracle vs planted oracle >= 4 bounds) and of the tap bound
    (device vs oracle <= 1 bound): the device's tap l lies >= 3 bounds from the oracle with ANY of the 45 observable plants in
    layer l, on the 33- and 129-frame utterances.  A kernel with that error would sit where the planted oracle sits."""
    ref, got = run["ref"], run["got"]
    audio, lens = _batch()
    against = {l: got["taps"][f"layer{l}"][PLANT_ROWS] for l in range(R.N_LAYERS)}
    plants = {k: p for k, p in FR.PLANTS.items() if k != FR.BLIND}
    power = FR.layer_power(_weights(run["kind"]), audio, lens, PLANT_ROWS, against=against, plants=plants)
    assert power["t"] == [FRAMES[r] for r in PLANT_ROWS]
    ratios = sorted((d / ref["bound_tap"][l], key, l) for key, row in power["A"].items() for l, d in enumerate(row))
    assert len(ratios) == 45 * R.N_LAYERS
    for l in range(R.N_LAYERS):
        r, key = min((row[l] / ref["bound_tap"][l], key) for key, row in power["A"].items())
        print(f"[layer-taps] precision {run['precision']} layer {l:2d}: nearest planted oracle {r:.2f} bounds away ({key})")
    print(f"[layer-taps] precision {run['precision']}: smallest ratio {ratios[0][0]:.2f} bounds: {ratios[0][1]} in layer {ratios[0][2]}")
    low = [(key, l, round(r, 2)) for r, key, l in ratios if r < 3.0]
    assert not low, low
