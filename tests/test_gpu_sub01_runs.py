"""k_sub01 walks a run of four-frame tiles per block (GPU): its own output (the c1 tap) and the log-probs against the
two-kernel path (QVERSE_SUB_UNFUSED=1: k_conv0 + k_dwconv2d through HBM), bit for bit.

  * clips whose c1 frame counts are EVERY value from 1 to 2 x (the longest run a block ever walks, in frames) + 1: the
    400-sample minimum, counts that are no multiple of four, counts that end on, one short of and one past every run
    boundary.  Sample counts come from the engine's own frame arithmetic (Engine.sub01_plan), shortest clip per count;
  * packed into ragged batches of 16 with a short clip beside a long one, so blocks see rows past an utterance's end;
  * the run length forced to 1 tile, 2 tiles and the maximum through kernel_variant(5, .): no bit changes;
  * a clip with a partial last tile alone, as the first and as the last row of a ragged batch;
  * 30 s clips (the longest runs the default choice takes) beside a 1 s clip.

The two-kernel results are computed once per module and never modified."""

import os

import pytest
import torch

from synth import synth_audio

pytestmark = pytest.mark.gpu

SEED = 7
KV_SUB_RUN = 5
_cache = {}


def _engine(max_batch, max_samples, unfused):
    from offline_tarteel_amd.engine import Engine

    old = os.environ.pop("QVERSE_SUB_UNFUSED", None)
    if unfused:
        os.environ["QVERSE_SUB_UNFUSED"] = "1"
    try:
        return Engine(device=0, with_model=True, seed=SEED, max_batch=max_batch, max_samples=max_samples)
    finally:
        os.environ.pop("QVERSE_SUB_UNFUSED", None)
        if old is not None:
            os.environ["QVERSE_SUB_UNFUSED"] = old


def _samples_by_c1_frames(eng, up_to):
    """c1 frame count -> the shortest clip (in samples, hop by hop from the 400-sample minimum) that has it"""
    table, n = {}, 400
    while len(table) < up_to:
        table.setdefault(eng.sub01_plan(n)["c1"], n)
        n += 160 if n > 400 else 80
        assert n < 64 * 160 * (up_to + 2), "frame counts are not contiguous"
    assert sorted(table) == list(range(1, up_to + 1)), sorted(table)
    return table


def _run(eng, audio, lens):
    """(c1 tap, log-probs, frames) of one forward, cloned"""
    lp, t = eng.forward(audio, lens)
    torch.cuda.synchronize()
    c1 = eng.forward_tap(eng.TAP_C1, 0, batch=len(lens), c1_frames=max(eng.sub01_plan(n)["c1"] for n in lens))
    return c1.clone(), lp.clone(), list(t)


def _assert_same(eng, lens, got, want, what):
    assert got[2] == want[2], what
    for b, n in enumerate(lens):
        f = eng.sub01_plan(n)["c1"]
        assert torch.equal(got[0][b, :f], want[0][b, :f]), (what, "c1", b, n, f)
        assert torch.equal(got[1][b, : got[2][b]], want[1][b, : want[2][b]]), (what, "log-probs", b, n)
        assert bool(torch.isfinite(got[0][b, :f]).all())


@pytest.fixture(scope="module")
def ladder():
    """the fused engine, the ragged batches and what the two-kernel path gives for them"""
    from offline_tarteel_amd.engine import Engine

    probe = Engine(device=0, with_model=False, max_batch=1, max_samples=16000)      # frame arithmetic only
    try:
        probe.kernel_variant(KV_SUB_RUN, 3)
        max_run = probe.sub01_plan(16000 * 60, 16)["run_tiles"]      # the most tiles a block ever walks
        probe.kernel_variant(KV_SUB_RUN, -1)
        top = 2 * 4 * max_run + 1
        samples = _samples_by_c1_frames(probe, top)
    finally:
        probe.kernel_variant(KV_SUB_RUN, -1)
        probe.close()
    assert samples[1] == 400
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
        audio = noise[: len(lens), : max(lens)].clone()
        for b, n in enumerate(lens):
            audio[b, n:] = 0
        batches.append((audio.cuda().contiguous(), lens))
    ref = _engine(16, cap, True)
    try:
        want = [_run(ref, a, l) for a, l in batches]
    finally:
        ref.close()
    eng = _engine(16, cap, False)
    yield {"eng": eng, "batches": batches, "want": want, "max_run": max_run, "top": top, "samples": samples}
    eng.kernel_variant(KV_SUB_RUN, -1)
    eng.close()


def test_fused_equals_two_kernel_path_at_every_frame_count(ladder):
    eng = ladder["eng"]
    assert ladder["max_run"] >= 2 and ladder["top"] == 8 * ladder["max_run"] + 1
    seen = set()
    for (audio, lens), want in zip(ladder["batches"], ladder["want"]):
        _assert_same(eng, lens, _run(eng, audio, lens), want, "default run length")
        seen.update(eng.sub01_plan(n)["c1"] for n in lens)
    assert seen == set(range(1, ladder["top"] + 1))


def test_run_length_changes_nothing(ladder):
    eng = ladder["eng"]
    try:
        for audio, lens in ladder["batches"]:
            eng.kernel_variant(KV_SUB_RUN, -1)
            base = _run(eng, audio, lens)
            runs = {}
            for mode in (1, 2, 3):
                eng.kernel_variant(KV_SUB_RUN, mode)
                runs[mode] = eng.sub01_plan(max(lens), len(lens))["run_tiles"]
                _assert_same(eng, lens, _run(eng, audio, lens), base, f"run length mode {mode}")
            n_tiles = (eng.sub01_plan(max(lens))["c1"] + 3) // 4
            assert runs == {1: 1, 2: min(2, n_tiles), 3: min(ladder["max_run"], n_tiles)}, runs
    finally:
        eng.kernel_variant(KV_SUB_RUN, -1)
    # the knob is part of what the forward is keyed on: the default is back
    audio, lens = ladder["batches"][0]
    _assert_same(eng, lens, _run(eng, audio, lens), ladder["want"][0], "default after the knob")


def test_batch_invariance_at_a_partial_last_tile(ladder):
    eng, samples = ladder["eng"], ladder["samples"]
    f = 4 * 6 + 3                                   # six full tiles and three frames of the seventh
    n = samples[f]
    others = [samples[g] for g in (ladder["top"], 1, 4 * 6, 2 * 4 * 2 + 1)]
    cap = max(others + [n])
    noise = torch.from_numpy(synth_audio(5, cap))
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
    t = alone[2][0]
    assert got_first[2][0] == t and got_last[2][4] == t
    for got, row in ((got_first, 0), (got_last, 4)):
        assert torch.equal(got[0][row, :f], alone[0][0, :f]), row
        assert torch.equal(got[1][row, :t], alone[1][0, :t]), row


def test_long_clips_beside_a_short_one():
    lens = [480000, 480000, 16000]
    audio = torch.from_numpy(synth_audio(3, 480000))
    for b, n in enumerate(lens):
        audio[b, n:] = 0
    audio = audio.cuda().contiguous()
    ref = _engine(3, 480000, True)
    try:
        want = _run(ref, audio, lens)
    finally:
        ref.close()
    eng = _engine(3, 480000, False)
    try:
        assert eng.sub01_plan(480000, 3)["run_tiles"] >= 1
        _assert_same(eng, lens, _run(eng, audio, lens), want, "30 s")
    finally:
        eng.close()
