"""The HIP forward against its reference at every length it accepts (GPU), on weights where an error would show.

What the other forward tests leave open: nothing beyond 30 s (T = 376) is run through the model although an engine takes
61 s (T = 766); between 129 and 375 frames the forward is only compared with itself; and on the seeded random weights the
attention's relative-position term moves the log-probs by less than the 1e-2 every oracle comparison grants.  Here:

  * weights: "sharp attention" (forward_ref.sharp_weights: the query side x4) from a weight file -- a position off-by-one
    or a dropped last key frame moves the log-probs by 6-40x the bound there, which test_planted_errors_* shows with the
    ORACLE computing the wrong thing, never a kernel; the plain seeded weights and the structured (peaked) set as well;
  * lengths: the tile-edge ladder 1 .. 257 and the batch 766 / 513 / 417 / 385 / 377 / 129 of an engine for 979,200 samples;
  * bounds, one rule (forward_ref.check_rules): e = max |twin - fp32 oracle| per utterance, where the twin is the oracle
    with float16 operands in every Linear / Conv -- (a) device vs fp32 <= max(1e-2, 1.5 e).  Rule (b), device vs twin <= e,
    did not hold on the device (up to 1.04 e; 1.13 e from the twin extended by the attention kernels' roundings, with every
    tap in line): its distance is printed, not asserted.

Oracle results are computed once per module (the `_cached` table) and never modified."""

import math
import os

import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R
from ort_floor import _assert_on_the_floor, delta, oracle_floor

pytestmark = pytest.mark.gpu

SEED = 7
CHECKED = {"ladder": [33, 129, 257], "long": [417, 766]}     # utterances the planted errors are evaluated on
TAP_LAYERS = {"ladder": (0, 8, 16), "long": (0, 16)}
_cache = {}


def _cached(key, make):
    if key not in _cache:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _cache[key] = make()
    return _cache[key]


def _weights(kind):
    """'plain' (the engine's seeded init), 'sharp', 'sharp_q' (what a precision-1 engine makes of the sharp file), 'structured'"""
    def make():
        if kind == "plain":
            return R.random_weights(SEED)
        if kind == "sharp":
            return FR.sharp_weights(_weights("plain"))
        if kind == "sharp_q":
            return R.quantize_linear_weights(_weights("sharp"))
        return R.structured_weights(SEED)
    return _cached(("w", kind), make)


def _batch(name):
    def make():
        if name == "ladder":
            lens = [FR.samples_for_frames(t) for t in FR.LADDER]
            return FR.clips(lens, FR.LADDER_AUDIO_SEED), lens
        lens = FR.long_lens()
        return FR.clips(lens, FR.LONG_AUDIO_SEED), lens
    return _cached(("audio", name), make)


def _ref(name, kind):
    audio, lens = _batch(name)
    taps = ["sub"] + [f"layer{l}" for l in TAP_LAYERS[name]] if kind != "plain" else None
    return _cached(("ref", name, kind), lambda: FR.reference(_weights(kind), audio, lens, taps=taps))


def _engine(taps=False, **kw):
    from offline_tarteel_amd.engine import Engine

    if not taps:
        return Engine(device=0, with_model=True, **kw)
    os.environ["QVERSE_DEBUG_TAPS"] = "1"      # read when the engine is created
    try:
        return Engine(device=0, with_model=True, **kw)
    finally:
        os.environ.pop("QVERSE_DEBUG_TAPS", None)


def _forward(eng, dev, lens, variant=None):
    if variant is not None:
        eng.attention_variant(variant)
    try:
        lp, t = eng.forward(dev, lens)
        torch.cuda.synchronize()
        return lp, t
    finally:
        if variant is not None:
            eng.attention_variant(-1)


def _same_rows(a, b, t):
    return [bool(torch.equal(a[i, :n], b[i, :n])) for i, n in enumerate(t)]


@pytest.fixture(scope="module")
def weight_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("forward_lengths")


@pytest.fixture(scope="module")
def sharp_file(weight_dir):
    return FR.write_weights(weight_dir / "sharp.qvw", _weights("sharp"))


def _taps_of(eng, name, B, T):
    return {"sub": eng.forward_tap(1, 0, (B, T, 512)).cpu(),
            **{f"layer{l}": eng.forward_tap(2, l, (B, T, 512)).cpu() for l in TAP_LAYERS[name]}}


@pytest.fixture(scope="module", params=[0, 1], ids=["precision0", "precision1"])
def ladder(request, sharp_file):
    """everything the device computes for the ladder, in one engine's lifetime; the tests below only compare"""
    p = request.param
    audio, lens = _batch("ladder")
    ref = _ref("ladder", "sharp_q" if p else "sharp")
    eng = _engine(taps=True, weights_path=str(sharp_file), precision=p, max_batch=len(lens), max_samples=max(lens))
    try:
        dev = audio.cuda().contiguous()
        lp, t = _forward(eng, dev, lens)
        got = {"lp": lp.cpu(), "t": t, "taps": _taps_of(eng, "ladder", len(lens), max(t))}
        if p == 0:
            got["lp_tiled"] = _forward(eng, dev, lens, variant=0)[0].cpu()     # the key-tiled kernel at 1-128 frames as well
    finally:
        eng.close()
    return dict(name="ladder", precision=p, kind="sharp_q" if p else "sharp", ref=ref, got=got)


@pytest.fixture(scope="module", params=[0, 1], ids=["precision0", "precision1"])
def long(request, sharp_file):
    """the batch beyond 30 s on an engine for the longest clip qv_create accepts"""
    from offline_tarteel_amd.engine import QvError

    p = request.param
    audio, lens = _batch("long")
    ref = _ref("long", "sharp_q" if p else "sharp")
    eng = _engine(taps=True, weights_path=str(sharp_file), precision=p, max_batch=6, max_samples=FR.MAX_SAMPLES)
    try:
        dev = audio.cuda().contiguous()
        lp, t = _forward(eng, dev, lens)
        got = {"lp": lp.cpu(), "t": t, "taps": _taps_of(eng, "long", len(lens), max(t))}
        got["alone"] = []
        for b, n in enumerate(lens):
            one, t1 = _forward(eng, dev[b: b + 1, :n].contiguous(), [n])
            got["alone"].append(t1[0] == t[b] and bool(torch.equal(one[0, : t[b]], lp[b, : t[b]])))
        if p == 0:
            tiled = {v: _forward(eng, dev, lens, variant=v)[0] for v in (0, 1, 2, 4)}
            got["tiled_same"] = {v: _same_rows(tiled[v], tiled[0], t) for v in (1, 2, 4)}
            got["tiled_is_default"] = _same_rows(tiled[0], lp, t)
            got["variant5_same"] = _same_rows(_forward(eng, dev, lens, variant=5)[0], lp, t)
        got["predict"] = eng.predict_batch(dev, lens)
        try:
            eng.forward(torch.zeros(1, FR.MAX_SAMPLES + 1, device="cuda"), [FR.MAX_SAMPLES + 1])
            got["refused"] = False
        except QvError:
            got["refused"] = True
        lp2, t2 = _forward(eng, dev, lens)                         # ... and the refusal left the engine as it was
        got["after_refusal"] = t2 == t and all(_same_rows(lp2, lp, t))
    finally:
        eng.close()
    return dict(name="long", precision=p, kind="sharp_q" if p else "sharp", ref=ref, got=got)


def _check_taps(run):
    ref, got, T = run["ref"], run["got"], run["got"]["t"]
    figures = {}
    for key, want in ref["taps"].items():
        scale = math.sqrt(512) if key == "sub" else 1.0             # the device keeps the xscaled tensor (values ~ +-30)
        figures[key] = max(FR.maxdiff(got["taps"][key][b], want[b] * scale, n) for b, n in enumerate(T))
        print(f"[fwd-len] {run['name']} precision {run['precision']} tap {key}: {figures[key]:.3e}")
    for key, d in figures.items():
        assert d <= (5e-2 if key == "sub" else 1.5e-2), (key, d)


def _check_sums(run):
    for b, n in enumerate(run["got"]["t"]):
        lp = run["got"]["lp"][b, :n]
        assert bool(torch.isfinite(lp).all()), n
        assert torch.allclose(lp.exp().sum(-1), torch.ones(n), atol=1e-4), n


# ------------------------------------------------------------------ 1. the ladder ---------------------------------------

def test_ladder_logprobs_on_sharp_weights(ladder):
    """frames 1 .. 257 ragged in one batch, weights from a file: frame counts, rule (a) per utterance, normalised
    posteriors; in precision 0 the same again with the key-tiled kernel serving every utterance (variant 0)."""
    ref, got = ladder["ref"], ladder["got"]
    assert got["t"] == ref["t"] == FR.LADDER
    FR.check_rules(f"ladder precision {ladder['precision']}", got["lp"], ref)
    _check_sums(ladder)
    if ladder["precision"] == 0:
        differ = sum(not torch.equal(got["lp_tiled"][b, :n], got["lp"][b, :n]) for b, n in enumerate(FR.LADDER) if n <= 128)
        assert differ >= 4      # another kernel did run there (a one-frame softmax is the same in any kernel)
        FR.check_rules("ladder precision 0, key-tiled kernel", got["lp_tiled"], ref)


def test_ladder_taps_on_sharp_weights(ladder):
    """subsampling output and layers 0, 8, 16 against the fp32 oracle, with the bounds of test_gpu_forward.py"""
    _check_taps(ladder)


# ------------------------------------------------------------------ 2. beyond 30 s --------------------------------------

def test_beyond_30s_logprobs_on_sharp_weights(long):
    """766 / 513 / 417 / 385 / 377 / 129 frames: the 24-key-tile attention loop, the 1,531-row position table, the position
    rings, t_pad of the V^T store -- rule (a) per utterance, layer taps 0 and 16."""
    ref, got = long["ref"], long["got"]
    assert got["t"] == ref["t"] == FR.LONG
    FR.check_rules(f"long precision {long['precision']}", got["lp"], ref)
    _check_sums(long)
    _check_taps(long)


def test_beyond_30s_batch_invariance_and_kernel_variants(long):
    got = long["got"]
    assert all(got["alone"]), got["alone"]                       # every utterance alone == its rows in the batch, bit for bit
    if long["precision"] == 0:
        for v, same in got["tiled_same"].items():                # key-tiled kernels 0, 1, 2, 4: identical bits
            assert all(same), (v, same)
        assert all(got["variant5_same"]), got["variant5_same"]   # k_attention_short + k_attention_x == the default
        # all six utterances are above 128 frames: the default serves them with a key-tiled kernel too
        assert all(got["tiled_is_default"]), got["tiled_is_default"]


def test_beyond_30s_whole_path(long, oracle):
    """predict_batch on the long batch: frame counts, and the post-logits path (long CTC / alignment instantiations above 384
    frames) equal to the oracle's on the device's own log-probs, as test_max_length_ragged_batch_30s compares them"""
    got = long["got"]
    assert [r["t_frames"] for r in got["predict"]] == FR.LONG
    for i, n in enumerate(got["t"]):
        want = oracle.predict_logprobs(got["lp"][i, :n].numpy())
        res = got["predict"][i]
        assert res["greedy_ids"] == want["greedy_ids"], n
        assert (res["surah"], res["ayah"], res["ayah_end"], res["source"]) == (
            want["surah"], want["ayah"], want["ayah_end"], want["source"]), n
        assert abs(res["score"] - want.get("score_raw", 0.0)) <= 1e-3 * max(want.get("score_raw", 0.0), 1e-3), n


def test_one_sample_beyond_the_capacity_is_refused(long):
    """979,201 samples on an engine for 979,200: the same number of mel frames, so every buffer would still fit -- but
    the contract is in samples (include/qverse.h: QV_ERR_CAPACITY)"""
    assert long["got"]["refused"]
    assert long["got"]["after_refusal"]


# ------------------------------------------------------------------ 3. what 1 and 2 would catch -------------------------

def test_planted_errors_would_fail_the_ladder(ladder):
    """The power of the tests above, shown without running a wrong kernel: the device's log-probs against the ORACLE with a
    planted error (relative positions off by one row; each utterance's last frame treated as padding).  A kernel with that
    error would sit where this oracle sits, and must then miss bound (a) by a wide margin: >= 4x."""
    _planted_check(ladder)


def test_planted_errors_would_fail_beyond_30s(long):
    _planted_check(long)


def _planted_check(run):
    name, ref, got = run["name"], run["ref"], run["got"]
    audio, lens = _batch(name)
    frames = FR.LADDER if name == "ladder" else FR.LONG
    rows = [frames.index(t) for t in CHECKED[name]]
    bad = _cached(("planted", name, run["kind"]), lambda: FR.planted(_weights(run["kind"]), audio, lens, rows))
    figures = []
    for b in rows:
        n = frames[b]
        d_pos = FR.maxdiff(got["lp"][b], bad["positions"][b], n)
        d_last = FR.maxdiff(got["lp"][b], bad["last_frame"][b], n - 1)          # all frames but the last
        figures.append((n, d_pos, d_last, ref["bound"][b]))
        print(f"[fwd-len] {name} precision {run['precision']} T={n}: device vs oracle with positions off by one {d_pos:.3f}, "
              f"with the last frame dropped {d_last:.3f}; bound (a) {ref['bound'][b]:.3e}")
    for n, d_pos, d_last, bound in figures:
        assert d_pos >= 4.0 * bound, (n, d_pos, bound)
        assert d_last >= 4.0 * bound, (n, d_last, bound)


# ------------------------------------------------------------------ 4. plain random weights beyond 30 s -----------------

def test_beyond_30s_on_the_seeded_random_weights():
    """the configuration every other forward test uses (seeded init, no file, precision 0), at the lengths none of them reaches"""
    audio, lens = _batch("long")
    ref = _ref("long", "plain")
    eng = _engine(seed=SEED, max_batch=6, max_samples=FR.MAX_SAMPLES)
    try:
        lp, t = _forward(eng, audio.cuda().contiguous(), lens)
        lp = lp.cpu()
    finally:
        eng.close()
    assert t == ref["t"] == FR.LONG
    FR.check_rules("long, seeded random weights", lp, ref)


# ------------------------------------------------------------------ 5. structured (peaked) weights ----------------------

def test_structured_weights(weight_dir):
    """peaked posteriors (max probability 0.6-0.8): the f16 operand rounding costs 3e-2 - 4e-2 there, so the bound is the
    twin's (rule (a): ~5e-2) and the decisions must be the oracle's wherever its top-1 / top-2 gap exceeds 4 e"""
    w = _weights("structured")
    lens = [FR.samples_for_frames(t) for t in FR.STRUCTURED_FRAMES]
    audio = FR.clips(lens, FR.STRUCTURED_AUDIO_SEED)
    ref = _cached(("ref", "structured"), lambda: FR.reference(w, audio, lens))
    eng = _engine(weights_path=str(FR.write_weights(weight_dir / "structured.qvw", w)), max_batch=3, max_samples=max(lens))
    try:
        lp, t = _forward(eng, audio.cuda().contiguous(), lens)
        lp = lp.cpu()
    finally:
        eng.close()
    assert t == ref["t"] == FR.STRUCTURED_FRAMES
    figures = []
    for b, n in enumerate(t):
        keep = FR.decided_frames(ref["lp"][b, :n], ref["e"][b])
        wrong = int(((lp[b, :n].argmax(-1) != ref["lp"][b, :n].argmax(-1)) & keep).sum())
        figures.append((n, 1.0 - float(keep.float().mean()), wrong))
        print(f"[fwd-len] structured T={n}: frames left out {figures[-1][1]:.3f}, decided frames with another argmax {wrong}, "
              f"mean max-probability {float(ref['lp'][b, :n].exp().max(-1).values.mean()):.3f}")
    FR.check_rules("structured weights", lp, ref)
    for n, left_out, wrong in figures:
        assert left_out <= 0.05, (n, left_out)
        assert wrong == 0, (n, wrong)


# ------------------------------------------------------------------ 6. precision 2 beyond 30 s --------------------------

def test_ort_mixed_beyond_30s():
    """the reference's int4 / dynamic-int8 arithmetic at 417 and 766 frames next to a one-frame clip: exact batch invariance,
    and the two long clips against OrtMixed, judged on its own floor (the protocol of
    test_edge_shapes_one_frame_thirty_seconds_and_silence)"""
    lens = [FR.samples_for_frames(417), FR.MAX_SAMPLES, 400]
    audio = FR.clips(lens, FR.LONG_AUDIO_SEED + 1)
    eng = _engine(seed=SEED, precision=2, max_batch=3, max_samples=FR.MAX_SAMPLES)
    try:
        dev = audio.cuda().contiguous()
        lp, T = _forward(eng, dev, lens)
        assert T == [417, 766, 1]
        for b, n in enumerate(lens):
            assert bool(torch.isfinite(lp[b, : T[b]]).all()), T[b]
            one, t1 = _forward(eng, dev[b: b + 1, :n].contiguous(), [n])
            assert t1[0] == T[b] and torch.equal(one[0, : T[b]], lp[b, : T[b]]), T[b]
        lp = lp.cpu()
    finally:
        eng.close()
    w = _weights("plain")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for b in (0, 1):
        one = audio[b: b + 1, : lens[b]].contiguous()
        ref, tr = R.forward(w, one, [lens[b]], ort=R.OrtMixed())
        assert int(tr[0]) == T[b]
        floor = oracle_floor(R, w, one, [lens[b]], ref, [T[b]], one_thread=False, seeds=(1, 2, 3), f16_inputs=True)
        _assert_on_the_floor(f"precision 2, T = {T[b]}", delta(lp[b: b + 1], ref, [T[b]]), floor)


# ------------------------------------------------------------------ 7. log-mel at the edge lengths ----------------------

def test_logmel_where_the_reflections_overlap():
    """the lengths of test_register_fft_logmel_equals_the_lds_kernel_bit_for_bit (reflection at both ends of a frame, the
    shortest clip), this time against the oracle's front end: 5e-4 on the valid frames, exact zeros behind them"""
    lens = [80000, 400, 401, 560, 799, 1000, 30001, 4000]
    audio = FR.clips(lens, 20260630)
    feats, tm = R.frontend(audio, torch.as_tensor(lens, dtype=torch.int64))
    want = feats.transpose(1, 2)                                    # what R.forward stores as taps["mel"]
    tm = tm.tolist()
    assert tm == [n // 160 + 1 for n in lens]
    eng = _engine(seed=SEED, max_batch=len(lens), max_samples=max(lens))
    try:
        _forward(eng, audio.cuda().contiguous(), lens)
        mel = eng.forward_tap(0, 0, (len(lens), max(tm), 80)).cpu()
    finally:
        eng.close()
    figures = [FR.maxdiff(mel[b], want[b], n) for b, n in enumerate(tm)]
    for n, d in zip(lens, figures):
        print(f"[fwd-len] log-mel, {n} samples: {d:.3e}")
    for b, d in enumerate(figures):
        assert d <= 5e-4, (lens[b], d)
        if tm[b] < max(tm):
            assert float(mel[b, tm[b]:].abs().max()) == 0.0, lens[b]
