"""The premises of tests/test_gpu_forward_isolation.py, checked with the reference alone (CPU, oracle/fastconformer_ref.py):
every poison kind of forward_ref.POISON_KINDS leaves its own row without a single finite log-prob (otherwise it would not be
poison: a kernel could read it and stay finite), a healthy row beside it in the same oracle batch is the row run alone, and
the "loud" row (a clip in unscaled int16 units) is finite in the fp32 oracle and in the f16-operand twin, with the twin's
distance `e` from the oracle where it is on a normal clip."""

import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R

SEED = 7
FRAMES = 33
N_LAYERS = 2            # a NaN that reaches the encoder stays one: two layers show what seventeen would


@pytest.fixture(scope="module")
def clips():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    n = FR.samples_for_frames(FRAMES)
    audio = FR.clips([n, n], FR.LADDER_AUDIO_SEED)
    w = R.random_weights(SEED)
    alone, t = R.forward(w, audio[:1], [n], n_layers=N_LAYERS)
    assert t.tolist() == [FRAMES] and bool(torch.isfinite(alone).all())
    return dict(n=n, audio=audio, w=w, alone=alone[0])


@pytest.mark.parametrize("kind", FR.POISON_KINDS)
def test_poison_kinds_are_poison_and_stay_in_their_row(clips, kind):
    n, audio = clips["n"], clips["audio"]
    bad = FR.poisoned(audio[1], n, kind)
    assert bool(torch.isfinite(bad).all()) == (kind == "huge")          # "huge" is the one kind with finite samples
    assert not bad[n:].any()
    lp, t = R.forward(clips["w"], torch.stack([audio[0], bad]), [n, n], n_layers=N_LAYERS)
    assert t.tolist() == [FRAMES, FRAMES]
    finite = int(torch.isfinite(lp[1]).sum())
    d = FR.maxdiff(lp[0], clips["alone"], FRAMES)
    print(f"[fwd-iso] {kind}: finite log-probs in its own row {finite} of {lp[1].numel()}, healthy neighbour vs alone {d:.2e}")
    assert finite == 0, (kind, finite)
    assert bool(torch.isfinite(lp[0]).all()), kind
    assert d <= 1e-5, (kind, d)                                         # the bound of test_oracle_is_batch_invariant


def test_loud_clip_is_finite_and_on_the_usual_floor(clips):
    """the clip times 32768: log-mel moves by a constant the per-feature normalisation removes, so the oracle, the twin and the
    twin's distance e stay where they are on the clip itself"""
    n, audio = clips["n"], clips["audio"]
    loud = FR.poisoned(audio[1], n, "loud").unsqueeze(0)
    assert float(loud.abs().max()) > 1e3 and bool(torch.isfinite(loud).all())
    ref = FR.reference(clips["w"], loud, [n])
    plain = FR.reference(clips["w"], audio[1:2].contiguous(), [n], twin=True)
    assert ref["t"] == [FRAMES]
    for key in ("lp", "twin", "twin_att"):
        assert bool(torch.isfinite(ref[key]).all()), key
    assert torch.allclose(ref["lp"][0].exp().sum(-1), torch.ones(FRAMES), atol=1e-4)
    d = FR.maxdiff(ref["lp"][0], plain["lp"][0], FRAMES)
    print(f"[fwd-iso] loud, T={FRAMES}: e {ref['e'][0]:.3e} (the clip itself: {plain['e'][0]:.3e}), bound (a) {ref['bound'][0]:.3e}, "
          f"oracle loud vs oracle plain {d:.3e}")
    assert 0.0 < ref["e"][0] < 1e-2, ref["e"][0]                         # "small": rule (a) = max(1e-2, 1.5 e) stays the project's 1e-2
