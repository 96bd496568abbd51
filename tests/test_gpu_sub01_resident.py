"""k_sub01 with the run's normalised mel rows resident in LDS (runs of at most four tiles) against the two-kernel path
(QVERSE_SUB_UNFUSED=1: k_conv0 + k_dwconv2d through HBM), bit for bit (GPU): the c1 tap as f32 and the log-probs.

  * ragged batches whose c1 frame counts are 1, 3, 4, 5 (one tile +- 1), 15, 16, 17 (one resident run of four tiles +- 1),
    31, 32, 33, 47, 49 and 65; sample counts come from the engine's own frame arithmetic, shortest clip per count;
  * one batch with the 1-frame clip first, one with it last, each time beside the 65-frame one: len1 zeroing, and runs
    that start past a short utterance's end;
  * each under the default choice and under forced runs of 1, 2 and 4 tiles (resident rows) and 16 tiles (the variant
    that refetches the mel rows per channel group);
  * a two-context engine whose third forward is a graph replay; one precision-1 engine.

The two-kernel results are computed once per module and never modified."""

import os

import pytest
import torch

from synth import synth_audio

pytestmark = pytest.mark.gpu

SEED = 7
KV_SUB_RUN = 5
RES_RUN = 4         # tiles a block walks at most with resident rows
MAX_RUN = 16        # tiles a block walks at most
COUNTS = [1, 65, 3, 49, 4, 47, 5, 33, 15, 32, 16, 31, 17]      # short beside long, the 1-frame clip first


def _engine(max_batch, max_samples, unfused, **kw):
    from offline_tarteel_amd.engine import Engine

    old = os.environ.pop("QVERSE_SUB_UNFUSED", None)
    if unfused:
        os.environ["QVERSE_SUB_UNFUSED"] = "1"
    try:
        return Engine(device=0, with_model=True, seed=SEED, max_batch=max_batch, max_samples=max_samples, **kw)
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


def _batch(noise, lens):
    audio = noise[: len(lens), : max(lens)].clone()
    for b, n in enumerate(lens):
        audio[b, n:] = 0
    return audio.cuda().contiguous()


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
def setup():
    from offline_tarteel_amd.engine import Engine

    probe = Engine(device=0, with_model=False, max_batch=1, max_samples=16000)      # frame arithmetic only
    try:
        samples = _samples_by_c1_frames(probe, max(COUNTS))
    finally:
        probe.close()
    assert samples[1] == 400
    cap = samples[max(COUNTS)]
    noise = torch.from_numpy(synth_audio(len(COUNTS), cap))
    batches = []
    for counts in (COUNTS, COUNTS[::-1]):           # the 1-frame clip first / last, the 65-frame one beside it
        lens = [samples[f] for f in counts]
        batches.append((_batch(noise, lens), lens))
    assert batches[0][1][0] == 400 and batches[1][1][-1] == 400
    ref = _engine(len(COUNTS), cap, True)
    try:
        want = [_run(ref, a, l) for a, l in batches]
        want_rows = ref.predict_batch(*batches[0], want_text=False)
    finally:
        ref.close()
    eng = _engine(len(COUNTS), cap, False)
    yield {"eng": eng, "batches": batches, "want": want, "want_rows": want_rows, "cap": cap}
    eng.kernel_variant(KV_SUB_RUN, -1)
    eng.close()


# knob value -> tiles per block it forces (None: the choice from the launch shape, which stays on the resident variant)
@pytest.mark.parametrize("mode,tiles", [(-1, None), (1, 1), (2, 2), (4, RES_RUN), (3, MAX_RUN)])
def test_c1_and_log_probs_equal_the_two_kernel_path(setup, mode, tiles):
    eng = setup["eng"]
    try:
        eng.kernel_variant(KV_SUB_RUN, mode)
        for (audio, lens), want in zip(setup["batches"], setup["want"]):
            run = eng.sub01_plan(max(lens), len(lens))["run_tiles"]
            n_tiles = (max(COUNTS) + 3) // 4
            assert (run == min(tiles, n_tiles)) if tiles else (1 <= run <= RES_RUN), (mode, run)
            _assert_same(eng, lens, _run(eng, audio, lens), want, f"run length mode {mode}")
    finally:
        eng.kernel_variant(KV_SUB_RUN, -1)


def test_two_contexts_graph_replay(setup):
    """the ragged batch three times through a two-context engine: the third forward replays the first one's graph"""
    audio, lens = setup["batches"][0]
    eng = _engine(len(COUNTS), setup["cap"], False, contexts=2)
    try:
        assert eng.sub01_plan(max(lens), len(lens))["run_tiles"] <= RES_RUN
        tickets = [eng.predict_batch_async(audio, lens) for _ in range(3)]
        rows = [eng.fetch_results(t, len(lens), eng.frames_for(max(lens))) for t in tickets]
        assert rows[0] == setup["want_rows"]
        assert rows[1] == rows[0] and rows[2] == rows[0]
        st = eng.forward_graph_stats()
        assert st["replays"] >= 1 and st["captures"] >= 1, st
    finally:
        eng.close()


def test_precision_1(setup):
    audio, lens = setup["batches"][1]
    ref = _engine(len(COUNTS), setup["cap"], True, precision=1)
    try:
        want = _run(ref, audio, lens)
    finally:
        ref.close()
    eng = _engine(len(COUNTS), setup["cap"], False, precision=1)
    try:
        assert eng.sub01_plan(max(lens), len(lens))["run_tiles"] <= RES_RUN
        _assert_same(eng, lens, _run(eng, audio, lens), want, "precision 1")
    finally:
        eng.close()
