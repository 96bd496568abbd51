"""k_sub35 (conv.3 + ReLU + conv.5 in one kernel, c2 written packed) against the four-launch path (QVERSE_SUB35_UNFUSED=1:
k_gemm256 + k_dwconv2d + k_gemm256 + k_pack_rows through HBM), bit for bit (GPU): the conv.5 output (tap 12, valid frames)
and the log-probs.

  * clips whose c2 frame counts are EVERY value from 1 to 2 x (the longest run a block ever walks, in frames) + 1: the
    400-sample minimum, counts that end on, one short of and one past every step (3 frames) and run boundary.  Sample
    counts come from the engine's own frame arithmetic, shortest clip per count: its c1 frame count is odd, so the last tap
    row of the 3x3 / s2 window falls on len2 and must be dropped;
  * packed into ragged batches of 16 with a short clip beside a long one;
  * the run length forced to 1 step, 2 steps and the maximum through kernel_variant(6, .): no bit changes;
  * a clip with a partial last step alone, as the first and as the last row of a ragged batch;
  * 30 s clips beside a 1 s clip; precision 1; a two-context engine whose third forward is a graph replay, then a second,
    differently ragged batch (row_map and the packed offsets are rewritten).

The four-launch results are computed once per module and never modified."""

import os

import pytest
import torch

from synth import synth_audio

pytestmark = pytest.mark.gpu

SEED = 7
KV_SUB35 = 6
STEP = 3            # c2 frames per step of k_sub35


def _engine(max_batch, max_samples, unfused, **kw):
    from offline_tarteel_amd.engine import Engine

    old = os.environ.pop("QVERSE_SUB35_UNFUSED", None)
    if unfused:
        os.environ["QVERSE_SUB35_UNFUSED"] = "1"
    try:
        return Engine(device=0, with_model=True, seed=SEED, max_batch=max_batch, max_samples=max_samples, **kw)
    finally:
        os.environ.pop("QVERSE_SUB35_UNFUSED", None)
        if old is not None:
            os.environ["QVERSE_SUB35_UNFUSED"] = old


def _frames(eng, n):
    return eng.sub01_plan(n)["frames"]


def _samples_by_c2_frames(eng, up_to):
    """c2 frame count -> the shortest clip (in samples, hop by hop from the 400-sample minimum) that has it"""
    table, n = {}, 400
    while len(table) < up_to:
        table.setdefault(_frames(eng, n), n)
        n += 160 if n > 400 else 80
        assert n < 64 * 160 * (up_to + 2), "frame counts are not contiguous"
    assert sorted(table) == list(range(1, up_to + 1)), sorted(table)
    return table


def _batch(noise, lens):
    audio = noise[: len(lens), : max(lens)].clone()
    for b, n in enumerate(lens):
        audio[b, n:] = 0
    return audio.cuda().contiguous()


def _run(eng, audio, lens):
    """(c2 tap, log-probs, frames) of one forward, cloned"""
    lp, t = eng.forward(audio, lens)
    torch.cuda.synchronize()
    c2 = eng.forward_tap(eng.TAP_C2, 0, shape=(len(lens), max(t), 10, 256))
    return c2.clone(), lp.clone(), list(t)


def _assert_same(eng, lens, got, want, what):
    assert got[2] == want[2], what
    for b, n in enumerate(lens):
        f = _frames(eng, n)
        assert f == got[2][b]
        assert torch.equal(got[0][b, :f], want[0][b, :f]), (what, "c2", b, n, f)
        assert not bool(got[0][b, f:].any()), (what, "c2 padding frames", b)
        assert torch.equal(got[1][b, :f], want[1][b, :f]), (what, "log-probs", b, n)
        assert bool(torch.isfinite(got[0][b, :f]).all())


@pytest.fixture(scope="module")
def ladder():
    """the fused engine, the ragged batches and what the four-launch path gives for them"""
    from offline_tarteel_amd.engine import Engine

    probe = Engine(device=0, with_model=False, max_batch=1, max_samples=16000)      # frame arithmetic only
    try:
        probe.kernel_variant(KV_SUB35, 3)
        max_run = probe.sub35_plan(16000 * 60, 16)["run_frames"]      # the most frames a block ever walks
        probe.kernel_variant(KV_SUB35, -1)
        top = 2 * max_run + 1
        samples = _samples_by_c2_frames(probe, top)
        odd_c1 = all(probe.sub01_plan(n)["c1"] % 2 == 1 for n in samples.values())
    finally:
        probe.kernel_variant(KV_SUB35, -1)
        probe.close()
    assert samples[1] == 400 and odd_c1
    cap = samples[top]
    # short beside long: 1, top, 2, top - 1, ...
    order = []
    lo, hi = 1, top
    while lo <= hi:
        order.append(lo)
        if hi != lo:
            order.append(hi)
        lo, hi = lo + 1, hi - 1
    noise = torch.from_numpy(synth_audio(16, cap))
    batches = []
    for i in range(0, len(order), 16):
        lens = [samples[f] for f in order[i:i + 16]]
        batches.append((_batch(noise, lens), lens))
    ref = _engine(16, cap, True)
    try:
        want = [_run(ref, a, l) for a, l in batches]
        want_rows = [ref.predict_batch(a, l, want_text=False) for a, l in batches[:2]]
    finally:
        ref.close()
    eng = _engine(16, cap, False)
    yield {"eng": eng, "batches": batches, "want": want, "want_rows": want_rows, "max_run": max_run, "top": top,
           "samples": samples, "noise": noise, "cap": cap}
    eng.kernel_variant(KV_SUB35, -1)
    eng.close()


def test_fused_equals_four_launch_path_at_every_frame_count(ladder):
    eng = ladder["eng"]
    assert ladder["max_run"] >= 2 * STEP and ladder["max_run"] % STEP == 0
    seen = set()
    for (audio, lens), want in zip(ladder["batches"], ladder["want"]):
        _assert_same(eng, lens, _run(eng, audio, lens), want, "default run length")
        seen.update(_frames(eng, n) for n in lens)
    assert seen == set(range(1, ladder["top"] + 1))


def test_run_length_changes_nothing(ladder):
    eng = ladder["eng"]
    try:
        for (audio, lens), want in zip(ladder["batches"], ladder["want"]):
            runs = {}
            for mode in (1, 2, 3):
                eng.kernel_variant(KV_SUB35, mode)
                runs[mode] = eng.sub35_plan(max(lens), len(lens))["run_frames"]
                _assert_same(eng, lens, _run(eng, audio, lens), want, f"run length mode {mode}")
            n_steps = (_frames(eng, max(lens)) + STEP - 1) // STEP
            assert runs == {1: STEP, 2: STEP * min(2, n_steps), 3: min(ladder["max_run"], STEP * n_steps)}, runs
    finally:
        eng.kernel_variant(KV_SUB35, -1)
    # the knob is part of what the forward is keyed on: the default is back
    audio, lens = ladder["batches"][0]
    _assert_same(eng, lens, _run(eng, audio, lens), ladder["want"][0], "default after the knob")


def test_batch_invariance_at_a_partial_last_step(ladder):
    eng, samples, noise = ladder["eng"], ladder["samples"], ladder["noise"]
    f = STEP * 6 + 1                                # six full steps and one frame of the seventh
    n = samples[f]
    while _frames(eng, n + 160) == f:               # the longest clip with that count: its c1 frame count is even
        n += 160
    assert _frames(eng, n) == f and eng.sub01_plan(n)["c1"] == 2 * f
    others = [samples[g] for g in (ladder["top"], 1, STEP * 6, 2 * STEP * 2 + 2)]
    clip = noise[4, :n].clone()

    def batch(lens, at):
        audio = noise[: len(lens), : max(lens)].clone()
        for b, m in enumerate(lens):
            audio[b, m:] = 0
        audio[at, :] = 0
        audio[at, :n] = clip
        return audio.cuda().contiguous()

    alone = _run(eng, batch([n], 0), [n])
    first = [n] + others
    last = others + [n]
    got_first = _run(eng, batch(first, 0), first)
    got_last = _run(eng, batch(last, 4), last)
    assert alone[2][0] == f and got_first[2][0] == f and got_last[2][4] == f
    for got, row in ((got_first, 0), (got_last, 4)):
        assert torch.equal(got[0][row, :f], alone[0][0, :f]), row
        assert torch.equal(got[1][row, :f], alone[1][0, :f]), row


@pytest.mark.parametrize("precision", [0, 1])
def test_long_clips_beside_a_short_one(precision):
    # precision 0: 30 s clips (the longest runs the default choice takes) beside a 1 s clip; precision 1: one ragged batch
    lens = [480000, 480000, 16000] if precision == 0 else [47920, 400, 16000, 33360, 80000]
    audio = _batch(torch.from_numpy(synth_audio(len(lens), max(lens))), lens)
    ref = _engine(len(lens), max(lens), True, precision=precision)
    try:
        want = _run(ref, audio, lens)
    finally:
        ref.close()
    eng = _engine(len(lens), max(lens), False, precision=precision)
    try:
        assert eng.sub35_plan(max(lens), len(lens))["run_frames"] >= STEP
        _assert_same(eng, lens, _run(eng, audio, lens), want, f"precision {precision}")
    finally:
        eng.close()


def test_two_contexts_graph_replay_and_a_second_ragged_batch(ladder):
    """the same ragged batch three times through a two-context engine (the third forward replays the first one's graph),
    then a differently ragged batch of the same size: every fetch equals the four-launch engine's rows"""
    (a0, l0), (a1, l1) = ladder["batches"][0], ladder["batches"][1]
    eng = _engine(16, ladder["cap"], False, contexts=2)
    try:
        tickets = [eng.predict_batch_async(a0, l0) for _ in range(3)]
        rows = [eng.fetch_results(t, len(l0), eng.frames_for(max(l0))) for t in tickets]
        assert rows[0] == ladder["want_rows"][0]
        assert rows[1] == rows[0] and rows[2] == rows[0]
        st = eng.forward_graph_stats()
        assert st["replays"] >= 1 and st["captures"] >= 1, st
        tickets = [eng.predict_batch_async(a1, l1) for _ in range(3)]
        rows = [eng.fetch_results(t, len(l1), eng.frames_for(max(l1))) for t in tickets]
        assert rows[0] == ladder["want_rows"][1]
        assert rows[1] == rows[0] and rows[2] == rows[0]
        # and the first batch again on a context that has meanwhile run the other one
        again = eng.fetch_results(eng.predict_batch_async(a0, l0), len(l0), eng.frames_for(max(l0)))
        assert again == ladder["want_rows"][0]
    finally:
        eng.close()
