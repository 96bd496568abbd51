"""k_logmel_run (QV_KV_LOGMEL 2: a wave walks a run of four frames, the mel projection runs over the run's 320 items)
against k_logmel_reg (1: one wave per frame) and the LDS kernel (0), bit for bit and without a tolerance (GPU): the raw
features (tap 0, the frames of each utterance) and the log-probs.

  * clips whose frame count tm = n / 160 + 1 is 3, 4, 5, 7, 8, 9, 15, 17 (four waves of a block +- 1) and 65 (four blocks
    and one frame): a partial last run, and the block boundary;
  * 400 (the engine's minimum), 401, 511, 512, 513 and 672 samples: reflection at both ends and the first sample inside
    one run;
  * the same clips beside a 10 s clip, in whose first and last runs frames with and without reflection alternate.

Each variant's results are computed once per module and never modified."""

import os

import pytest
import torch

from synth import synth_audio

pytestmark = pytest.mark.gpu

SEED = 7
KV_LOGMEL = 0
RUN = 4             # frames a wave of k_logmel_run walks
SHORT = [400, 401, 511, 512, 513, 672, 997, 1120, 1333, 2243, 2719, 10241]
TM = {3, 4, 5, 7, 8, 9, 4 * RUN - 1, 4 * RUN + 1, 16 * RUN + 1}
BATCHES = [SHORT, SHORT[::-1] + [160000], [160000] + SHORT, [10241, 400, 2243]]


CLIPS = SHORT + [160000]


def _batch(noise, lens):
    """clip n is the same audio in whatever row of whatever batch it sits"""
    audio = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        audio[b, :n] = noise[CLIPS.index(n), :n]
    return audio.cuda().contiguous()


@pytest.fixture(scope="module")
def results():
    """variant -> per batch (features, log-probs, frames)"""
    from offline_tarteel_amd.engine import Engine

    assert {n // 160 + 1 for n in SHORT} == TM
    os.environ["QVERSE_DEBUG_TAPS"] = "1"
    noise = torch.from_numpy(synth_audio(len(CLIPS), 160000))
    eng = Engine(device=0, with_model=True, seed=SEED, max_batch=len(CLIPS), max_samples=160000)
    got = {}
    try:
        for var in (0, 1, 2, -1):
            eng.kernel_variant(KV_LOGMEL, var)
            got[var] = []
            for lens in BATCHES:
                lp, t = eng.forward(_batch(noise, lens), lens)
                torch.cuda.synchronize()
                feats = eng.forward_tap(0, 0, (len(lens), max(lens) // 160 + 1, 80))
                got[var].append((feats.clone(), lp.clone(), list(t)))
    finally:
        eng.kernel_variant(KV_LOGMEL, -1)
        eng.close()
        os.environ.pop("QVERSE_DEBUG_TAPS", None)
    return got


@pytest.mark.parametrize("other", [1, 0, -1])
def test_run_walking_kernel_equals(results, other):
    """-1: the default choice gives what the run-walking kernel gives (it is the default)"""
    for lens, new, old in zip(BATCHES, results[2], results[other]):
        assert new[2] == old[2]
        for b, n in enumerate(lens):
            tm = n // 160 + 1
            assert torch.equal(new[0][b, :tm], old[0][b, :tm]), (other, "feats", b, n)
            assert bool(torch.isfinite(new[0][b, :tm]).all()), (b, n)
            assert torch.equal(new[1][b, : new[2][b]], old[1][b, : old[2][b]]), (other, "log-probs", b, n)


def test_a_clip_reads_the_same_in_every_batch(results):
    """the frames of a clip do not depend on its row or on the batch's longest clip (which decides the grid)"""
    new = results[2]
    for b, n in enumerate(SHORT):
        tm = n // 160 + 1
        assert torch.equal(new[0][0][b, :tm], new[1][0][len(SHORT) - 1 - b, :tm]), n
        assert torch.equal(new[0][0][b, :tm], new[2][0][b + 1, :tm]), n
    assert torch.equal(new[1][0][len(SHORT), :1001], new[2][0][0, :1001])
