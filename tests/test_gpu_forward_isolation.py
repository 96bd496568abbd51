"""Row and batch isolation of the forward under non-finite audio (GPU): what a row's log-probs may depend on.

Every other forward test feeds finite audio to a fresh engine, where a stale value times an exact zero is zero and a kernel
that reads memory nobody wrote in this run still looks right.  Here one batch of poison rows (forward_ref.POISON_KINDS: NaN,
+-inf, a power spectrum that overflows float32 -- tests/test_forward_isolation_host.py shows on the oracle that each leaves no
finite log-prob in its own row) goes through `Engine.forward`, and the healthy batches around it must not move by a bit:

  * history: H1, H2, H3 on the fresh engine, then the poison batch, then H1, H2, H3 again -- torch.equal on every valid frame,
    exact zeros behind them; under every attention kernel and GEMM tile policy, in all three precisions;
  * neighbours: healthy rows interleaved with poison rows in ONE batch == the same batch with benign rows in their place
    == each row alone;
  * replay: the same through the hipGraph replay of a two-context engine's predict_batch;
  * loud: a clip in unscaled int16 units (x 32768) is not poison -- finite, normalised, batch-invariant, on the oracle;
  * the ingest kernels (batched resampler, mixdown) with a NaN row beside healthy ones.

The batches: H1 = 1 / 33 / 65 / 129 / 257 / 100 frames (V^T pitch 288, the poison batch's), H2 = 33 / 65 / 31 (pitch 96),
H3 = 129 / 127 (pitch 160): every utterance but the one-frame one has V^T pad columns (frames T .. pad32(T) - 1 of the key
tile the attention kernels stage whole), both attention kernels run (<= 128 frames / above), and the pitch both equals and
differs from the poison batch's, so the pad columns alias what it wrote.  Poison only ever enters `forward`: the post-logits
entry points keep "valid frames hold no NaN" as their contract (include/qverse.h).

Measured: no test here fails on the kernels as they are, because no non-finite value gets past the front end --
conv.3's ReLU is a select that no NaN passes, precision 2's first quantiser makes integers of everything -- so the poison rows
come out as finite garbage and the encoder's stale reads multiply finite values by exact zeros.  The tests hold the end-to-end
statement, whatever keeps it true; a front end that propagates NaN would make the history test the one that fails."""

import contextlib

import numpy as np
import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R
from ort_floor import _assert_on_the_floor, delta, oracle_floor

pytestmark = pytest.mark.gpu

SEED = 7
CAP_FRAMES = 257
HEALTHY = {"H1": [1, 33, 65, 129, 257, 100], "H2": [33, 65, 31], "H3": [129, 127]}
AUDIO_SEED = {"H1": 3101, "H2": 3102, "H3": 3103, "poison": 3104, "benign": 3105, "loud": 3106}
P_KINDS = FR.POISON_KINDS + ("nan",)             # six rows of 257 frames: one of each kind and one more all-NaN row
NEIGHBOUR_ROWS = [(1, "nan"), (3, "huge"), (4, "pos_inf")]      # H1's rows of 33 / 129 / 257 frames, each followed by a poison row
LOUD_FRAMES = [33, 129]                          # one row per attention kernel
_cache = {}


def _cached(key, make):
    if key not in _cache:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _cache[key] = make()
    return _cache[key]


def _healthy(name):
    def make():
        lens = [FR.samples_for_frames(t) for t in HEALTHY[name]]
        return FR.clips(lens, AUDIO_SEED[name]), lens
    return _cached(("healthy", name), make)


def _poison_batch():
    def make():
        n = FR.samples_for_frames(CAP_FRAMES)
        base = FR.clips([n] * len(P_KINDS), AUDIO_SEED["poison"])
        return torch.stack([FR.poisoned(base[b], n, kind) for b, kind in enumerate(P_KINDS)]), [n] * len(P_KINDS)
    return _cached("poison", make)


def _neighbour_batches():
    """(benign, poisoned, lens, healthy rows, poison rows): H1's 33 / 129 / 257-frame rows, each followed by a row of the same
    length that is a normal clip in `benign` and poison in `poisoned`"""
    def make():
        h1, h1_lens = _healthy("H1")
        lens = [h1_lens[r] for r, _ in NEIGHBOUR_ROWS for _ in (0, 1)]
        other = FR.clips(lens, AUDIO_SEED["benign"])
        benign, bad = torch.zeros(len(lens), max(lens)), torch.zeros(len(lens), max(lens))
        for i, (r, kind) in enumerate(NEIGHBOUR_ROWS):
            n = h1_lens[r]
            benign[2 * i, :n] = bad[2 * i, :n] = h1[r, :n]
            benign[2 * i + 1] = other[2 * i + 1]
            bad[2 * i + 1] = FR.poisoned(other[2 * i + 1], n, kind)
        return benign, bad, lens, [0, 2, 4], [1, 3, 5]
    return _cached("neighbours", make)


def _loud_batch():
    """loud 33 frames / healthy 65 / loud 129; the oracle side holds the two loud rows only"""
    def make():
        lens = [FR.samples_for_frames(t) for t in (LOUD_FRAMES[0], 65, LOUD_FRAMES[1])]
        audio = FR.clips(lens, AUDIO_SEED["loud"])
        for b in (0, 2):
            audio[b] = FR.poisoned(audio[b], lens[b], "loud")
        return audio, lens
    return _cached("loud", make)


def _loud_ref(kind):
    """FR.reference of the two loud rows on the seeded weights ('plain') / on what a precision-1 engine makes of them ('plain_q')"""
    def make():
        audio, lens = _loud_batch()
        w = R.random_weights(SEED)
        if kind == "plain_q":
            w = R.quantize_linear_weights(w)
        sub_lens = [lens[0], lens[2]]
        return FR.reference(w, audio[[0, 2]][:, : max(sub_lens)].contiguous(), sub_lens)
    return _cached(("loud_ref", kind), make)


def _engine(precision, **kw):
    from offline_tarteel_amd.engine import Engine

    return Engine(device=0, with_model=True, seed=SEED, precision=precision, max_batch=6,
                  max_samples=FR.samples_for_frames(CAP_FRAMES), **kw)


def _forward(eng, dev, lens):
    lp, t = eng.forward(dev, lens)
    torch.cuda.synchronize()
    return lp, t


def _alone(eng, dev, lens, b):
    lp, t = _forward(eng, dev[b: b + 1, : lens[b]].contiguous(), [lens[b]])
    return lp[0], t[0]


def _same_rows(a, b, t):
    return [bool(torch.equal(a[i, :n], b[i, :n])) for i, n in enumerate(t)]


def _pad_is_zero(lp, t):
    return [bool((lp[i, n:] == 0).all()) for i, n in enumerate(t)]


def _not_finite(lp, t):
    return [int((~torch.isfinite(lp[i, :n])).sum()) for i, n in enumerate(t)]


@contextlib.contextmanager
def _switch(eng, setting):
    """one process-wide kernel switch for the forwards inside, restored behind them"""
    what, mode = setting
    knob = {"attention_variant": eng.attention_variant, "gemm_tiles": eng.gemm_tiles}.get(what)
    if knob:
        knob(mode)
    try:
        yield
    finally:
        if knob:
            knob(-1)


def _settings(precision):
    out = [("default", -1)]
    if precision == 0:
        out += [("attention_variant", 0), ("attention_variant", 2)]     # the key-tiled kernels for every utterance: loader waves / from global memory
    return out + [("gemm_tiles", 2), ("gemm_tiles", 0)]


# ------------------------------------------------------------------ 1. history ------------------------------------------

@pytest.fixture(scope="module", params=[0, 1, 2], ids=["precision0", "precision1", "precision2"])
def history(request):
    """everything the device computes in one engine's lifetime: the healthy batches under every setting on the FRESH engine,
    then per setting the poison batch and the healthy batches again.  The tests below only compare."""
    p = request.param
    eng = _engine(p)
    out = {"precision": p, "runs": {}}
    try:
        dev = {name: (_healthy(name)[0].cuda().contiguous(), _healthy(name)[1]) for name in HEALTHY}
        poison, poison_lens = _poison_batch()
        poison = poison.cuda().contiguous()
        fresh = {}
        for setting in _settings(p):
            with _switch(eng, setting):
                fresh[setting] = {name: _forward(eng, *dev[name]) for name in HEALTHY}
        for setting in _settings(p):
            with _switch(eng, setting):
                lp_p, t_p = _forward(eng, poison, poison_lens)
                run = {"poison_t": t_p, "poison_finite": [int(torch.isfinite(lp_p[b]).sum()) for b in range(len(P_KINDS))]}
                for name in HEALTHY:
                    lp, t = _forward(eng, *dev[name])
                    lp0, t0 = fresh[setting][name]
                    run[name] = {"t": t, "t_fresh": t0, "same": _same_rows(lp, lp0, t0), "pad_zero": _pad_is_zero(lp, t0),
                                 "not_finite": _not_finite(lp, t0), "fresh_not_finite": _not_finite(lp0, t0)}
            out["runs"][setting] = run
    finally:
        eng.attention_variant(-1)
        eng.gemm_tiles(-1)
        eng.close()
    return out


def test_healthy_batches_after_a_poison_batch_equal_the_fresh_engine(history):
    """a batch of NaN / inf / overflowing rows must leave nothing behind on the context: H1 (the poison batch's V^T pitch),
    H2 and H3 (other pitches) afterwards == the same batches on the fresh engine, bit for bit, with exact zeros behind every
    utterance -- under the default kernels, the key-tiled attention kernels for every utterance (precision 0) and both GEMM
    tile policies, each against its own pre-poison bits"""
    figures = []
    for setting, run in history["runs"].items():
        for name, frames in HEALTHY.items():
            r = run[name]
            figures.append((setting, name, r))
            print(f"[fwd-iso] precision {history['precision']} {setting[0]} {setting[1]} {name}: frames {r['t']}, rows equal to the fresh "
                  f"engine's {r['same']}, non-finite values per row {r['not_finite']} (fresh: {r['fresh_not_finite']}), zero padding {r['pad_zero']}")
    for setting, name, r in figures:
        assert r["t"] == r["t_fresh"] == HEALTHY[name], (setting, name)
        assert r["fresh_not_finite"] == [0] * len(r["t"]), (setting, name, r["fresh_not_finite"])
        assert all(r["same"]), (setting, name, r["same"], r["not_finite"])
        assert all(r["pad_zero"]), (setting, name, r["pad_zero"])


def test_the_poison_batch_reports_the_frame_counts_of_its_lengths(history):
    """frame counts come from the lengths, never from the samples.  What the poison rows' valid frames hold is unspecified
    (precision 2's quantisers turn a NaN into an integer; a ReLU on float16 bits may clear one): how many of their values
    were finite on the device is printed, not asserted"""
    for setting, run in history["runs"].items():
        print(f"[fwd-iso] precision {history['precision']} {setting[0]} {setting[1]}: finite log-probs per poison row "
              f"{list(zip(P_KINDS, run['poison_finite']))} of {CAP_FRAMES * 1025}")
    for setting, run in history["runs"].items():
        assert run["poison_t"] == [CAP_FRAMES] * len(P_KINDS), setting


# ------------------------------------------------------------------ 2. neighbours, loud ---------------------------------

@pytest.fixture(scope="module", params=[0, 1, 2], ids=["precision0", "precision1", "precision2"])
def side(request):
    """a second engine per precision, in this order: the loud batch and its rows alone (nothing non-finite has been through the
    context yet), the neighbour rows alone, the benign neighbour batch, the poisoned one"""
    p = request.param
    eng = _engine(p)
    out = {"precision": p}
    try:
        audio, lens = _loud_batch()
        dev = audio.cuda().contiguous()
        lp, t = _forward(eng, dev, lens)
        alone = [_alone(eng, dev, lens, b) for b in range(len(lens))]
        out["loud"] = {"lp": lp.cpu(), "t": t, "alone": [t1 == t[b] and bool(torch.equal(one[: t[b]], lp[b, : t[b]]))
                                                          for b, (one, t1) in enumerate(alone)]}
        benign, bad, lens, healthy, poison = _neighbour_batches()
        dev_benign, dev_bad = benign.cuda().contiguous(), bad.cuda().contiguous()
        alone = {b: _alone(eng, dev_benign, lens, b) for b in healthy}
        lp_benign, t_benign = _forward(eng, dev_benign, lens)
        lp_bad, t_bad = _forward(eng, dev_bad, lens)
        out["neighbours"] = {
            "t_benign": t_benign, "t_bad": t_bad,
            "benign_is_alone": [alone[b][1] == t_benign[b] and bool(torch.equal(alone[b][0][: t_benign[b]], lp_benign[b, : t_benign[b]])) for b in healthy],
            "bad_is_benign": [bool(torch.equal(lp_bad[b, : t_benign[b]], lp_benign[b, : t_benign[b]])) for b in healthy],
            "bad_is_alone": [bool(torch.equal(lp_bad[b, : t_benign[b]], alone[b][0][: t_benign[b]])) for b in healthy],
            "not_finite": _not_finite(lp_bad, t_benign), "pad_zero": _pad_is_zero(lp_bad, t_benign),
            "benign_pad_zero": _pad_is_zero(lp_benign, t_benign)}
    finally:
        eng.close()
    return out


def test_healthy_rows_beside_poison_rows_equal_themselves_alone(side):
    """one batch, healthy and poison rows alternating (33 / 129 / 257 frames; all-NaN, overflowing, one +inf sample): the
    healthy rows == the batch with benign clips in the poison rows' places == each of them alone; a poison row reports the
    frame count of its length and holds exact zeros behind it"""
    r = side["neighbours"]
    frames = [HEALTHY["H1"][row] for row, _ in NEIGHBOUR_ROWS for _ in (0, 1)]
    print(f"[fwd-iso] precision {side['precision']} neighbours: frames {r['t_bad']}, healthy rows equal to the benign batch's {r['bad_is_benign']}, "
          f"to themselves alone {r['bad_is_alone']}, non-finite values per row {r['not_finite']}, zero padding {r['pad_zero']}")
    assert r["t_benign"] == r["t_bad"] == frames
    assert all(r["benign_is_alone"]), r["benign_is_alone"]
    assert all(r["bad_is_benign"]), (r["bad_is_benign"], r["not_finite"])
    assert all(r["bad_is_alone"]), r["bad_is_alone"]
    assert all(r["pad_zero"]) and all(r["benign_pad_zero"]), (r["pad_zero"], r["benign_pad_zero"])


def test_a_loud_clip_is_not_poison(side):
    """a clip times 32768 (int16 units that nobody scaled), at 33 and 129 frames beside a healthy row: finite, normalised
    posteriors, the same bits alone, and on the oracle by the project's rule -- forward_ref.check_rules' (a) on the seeded
    weights in precisions 0 and 1 (e: test_forward_isolation_host.py prints 4.1e-3 at 33 frames, so the bound is the usual 1e-2),
    the OrtMixed floor of its own clip in precision 2 (tests/ort_floor.py as smoke() applies it, on the 33-frame row)"""
    p, got = side["precision"], side["loud"]
    audio, lens = _loud_batch()
    assert got["t"] == [LOUD_FRAMES[0], 65, LOUD_FRAMES[1]]
    assert all(got["alone"]), got["alone"]
    for b, n in enumerate(got["t"]):
        lp = got["lp"][b, :n]
        assert bool(torch.isfinite(lp).all()), n
        assert torch.allclose(lp.exp().sum(-1), torch.ones(n), atol=1e-4), n
    if p < 2:
        ref = _loud_ref("plain_q" if p else "plain")
        assert ref["t"] == LOUD_FRAMES
        FR.check_rules(f"loud, precision {p}", got["lp"][[0, 2]], ref)
    else:
        w = R.random_weights(SEED)
        one = audio[:1, : lens[0]].contiguous()
        ref, tr = R.forward(w, one, [lens[0]], ort=R.OrtMixed())
        assert tr.tolist() == [LOUD_FRAMES[0]]
        floor = oracle_floor(R, w, one, [lens[0]], ref, LOUD_FRAMES[:1], one_thread=False)
        _assert_on_the_floor(f"loud, precision 2, T = {LOUD_FRAMES[0]}", delta(got["lp"][:1], ref, LOUD_FRAMES[:1]), floor)


# ------------------------------------------------------------------ 3. through a graph replay ---------------------------

def test_a_poison_batch_between_two_graph_replays_changes_nothing():
    """predict_batch on a two-context engine replays H1's forward as one hipGraph launch once a context has captured it.  With
    a poison batch forwarded on that very context in between (plain launches: `forward` never replays), the next replay there
    must return every field of every row as before -- greedy ids of every frame, scores and CTC losses are functions of the
    context's log-prob workspace, which no entry point hands out -- and a plain forward of H1 the bits it had."""
    audio, lens = _healthy("H1")
    poison, poison_lens = _poison_batch()
    dev, poison = audio.cuda().contiguous(), poison.cuda().contiguous()
    eng = _engine(0, contexts=2)
    try:
        assert eng.contexts == 2
        lp0, t0 = _forward(eng, dev, lens)
        assert t0 == HEALTHY["H1"]
        want, replayed = None, {}
        for i in range(12):                                              # (a context captures a shape the second time it sees it)
            before = eng.forward_graph_stats()["replays"]
            res = eng.predict_batch(dev, lens, want_text=True)
            want = want or res
            assert res == want, i
            replayed[int(eng.lib.qv_last_context(eng.h))] = eng.forward_graph_stats()["replays"] == before + 1
            if len(replayed) == 2 and all(replayed.values()):
                break
        assert len(replayed) == 2 and all(replayed.values()), (replayed, eng.forward_graph_stats())
        assert [r["t_frames"] for r in want] == HEALTHY["H1"]
        k = int(eng.lib.qv_last_context(eng.h))
        _, t_p = _forward(eng, poison, poison_lens)                      # runs on the context of the last call
        assert int(eng.lib.qv_last_context(eng.h)) == k and t_p == [CAP_FRAMES] * len(P_KINDS)
        seen = []
        for _ in range(2):                                               # the contexts take turns: the second call is context k's
            before = eng.forward_graph_stats()["replays"]
            res = eng.predict_batch(dev, lens, want_text=True)
            seen.append(int(eng.lib.qv_last_context(eng.h)))
            assert eng.forward_graph_stats()["replays"] == before + 1, seen
            assert res == want, seen
        assert k in seen, (k, seen)
        assert eng.lib.qv_debug_forward_graph_failures(eng.h) == 0
        lp1, t1 = _forward(eng, dev, lens)
        assert int(eng.lib.qv_last_context(eng.h)) == k
        assert t1 == t0 and all(_same_rows(lp1, lp0, t0)), _not_finite(lp1, t0)
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. ingest kernels -----------------------------------

@pytest.fixture(scope="module")
def ingest():
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=2, max_samples=16000)
    yield eng
    eng.close()


@pytest.mark.parametrize("up,down", [(9, 10), (160, 441)])
def test_batched_resampler_keeps_a_nan_row_to_itself(ingest, up, down):
    """qv_upfirdn_batch: healthy rows beside an all-NaN row == the same call without it (the NaN row has a healthy row's
    length, so both calls use the same filter), and == the healthy call once more afterwards"""
    rng = np.random.default_rng(up * 1000 + down)
    lens = [44100, 30000, 12345]
    x = np.zeros((3, max(lens) + 13), dtype=np.float32)
    for r, n in enumerate(lens):
        x[r, :n] = (rng.standard_normal(n) * 0.3).astype(np.float32)
    with_nan = np.insert(x, 1, 0.0, axis=0)
    with_nan[1, : lens[1]] = np.nan
    want, n_want = ingest.resample_rows(torch.from_numpy(x).cuda(), lens, up, down)
    got, n_got = ingest.resample_rows(torch.from_numpy(with_nan).cuda(), [lens[0], lens[1]] + lens[1:], up, down)
    again, n_again = ingest.resample_rows(torch.from_numpy(x).cuda(), lens, up, down)
    torch.cuda.synchronize()
    assert n_got == [n_want[0], n_want[1]] + n_want[1:] and n_again == n_want
    assert bool(torch.isfinite(want).all()) and bool(torch.isnan(got[1, : n_got[1]]).all())
    assert torch.equal(got[[0, 2, 3]], want)
    assert not bool(got[1, n_got[1]:].any())                              # the zero padding up to the pitch, of the NaN row as well
    assert torch.equal(again, want)


def test_mixdown_keeps_a_nan_row_to_itself(ingest):
    channels, frames = 2, [1000, 777, 1]
    rng = np.random.default_rng(channels)
    x = np.zeros((3, max(frames) * channels), dtype=np.float32)
    for r, n in enumerate(frames):
        x[r, : n * channels] = (rng.standard_normal(n * channels) * 0.5).astype(np.float32)
    with_nan = np.insert(x, 1, 0.0, axis=0)
    with_nan[1, : frames[1] * channels] = np.nan
    want = ingest.mixdown_rows(torch.from_numpy(x).cuda(), frames, channels)
    got = ingest.mixdown_rows(torch.from_numpy(with_nan).cuda(), [frames[0], frames[1]] + frames[1:], channels)
    again = ingest.mixdown_rows(torch.from_numpy(x).cuda(), frames, channels)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and bool(torch.isnan(got[1, : frames[1]]).all())
    assert torch.equal(got[[0, 2, 3]], want)
    assert not bool(got[1, frames[1]:].any())
    assert torch.equal(again, want)
