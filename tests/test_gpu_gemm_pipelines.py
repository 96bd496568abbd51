"""Every pipeline variant of the 128- / 64-wide GEMM kernel (csrc/qv_gemm.hip) under a whole forward, bit for bit (GPU).

launch_shape instantiates k_gemm<EPI, BN, WQ, NST, LD> for both tile widths and both loader schemes (LD = 1: register
staging, two LDS stages, the default; LD = 0: direct global->LDS loads with 2, 3 or 4 stages and hand-counted vmcnt waits),
chosen by QVERSE_GEMM_LD / _NST / _NARROW.  The defaults reach 128-wide register staging for f16 weights and 64-wide
register staging for int4 weights only; everything else used to rest on a hand run.  Here qv_debug_gemm_pipeline walks the
variants in one process, qv_profile_replay_kernel says which kernel the launcher picks (gemm_kernel in qv_launch_plan.h: the
launcher and the name read the same function), and the log-probs must equal the default pipeline's as uint32 words: the
variants form the same f16 products with the same MFMA instruction and operand order, walk K in the same 16-deep steps and
dequantise on the consumer side -- only how a K-step's operands reach LDS differs.  The default path is itself held to the
fp32 oracle at these lengths by test_gpu_forward_lengths.py, so equal bits inherit that bound.

Inputs (per configuration): frames [1, 33, 129, 257] in one batch (420 packed rows: three full row tiles and one with 36
valid rows), [1] alone (M = 1: every row of the tile is clamped) and [128] alone (exactly one tile).  Every forward holds
every K of the model -- 256 (conv.6 as a GEMM: nk = 4, the four-stage edge), 512, 2048, 2560 (the subsampling projection) --
and every (weights, epilogue) pair of gemm_for_pair for f16 and int4 weights (checked against qv_model.hip):
  f16 weights, precision 0:  f16 (the position table), f16_swish (FFN-up), f16_relu (conv.6), resid (FFN-down, attention out,
                             pointwise_conv2), f32 (subsampling projection, CTC head), qkv, glu (pointwise_conv1)
  int4 weights, precision 1: f16 (the position table), f16_swish, resid, qkv; next to them f16 weights f16_relu / f32 and the
                             int8 pointwise convolutions (glu, resid), which only exist 128-wide with register staging
The position table is one GEMM per (T, pipeline) and engine: the forward caches it under the pipeline switches as well, so
the first forward of a configuration at each T runs the f16-epilogue kernel of that configuration.
Precision 2 is left out: its Linear layers are the int4 kernels of precision 1 and its convolutions are A8W8, which like
int8 ignores the three switches -- it launches no 128- / 64-wide kernel that precision 1 does not.

Configurations (CONFIGS), derived from launch_shape so that every instantiation it can reach for f16 and int4 weights is
launched; gemm_tiles(0) for the whole module, so that the 256 x 256 kernel takes no shape away:
  precision 0, ld 0, nst plan / 2 / 3 / 4, narrow plan   f16 128-wide lds2 / lds3 / lds4 (plan: 3 stages, 4 at K >= 1024)
  precision 0, ld 0, nst 2 / 3, narrow 1                 f16 64-wide lds2 / lds3 (GLU stays 128-wide)
  precision 0, ld 1, narrow 1                            f16 64-wide register staging
  precision 1, ld 1, narrow 0                            int4 128-wide register staging
  precision 1, ld 0, nst 2 / 3 / 4, narrow 0             int4 128-wide lds2 / lds3 / lds4
  precision 1, ld 0, nst 2 / 3, narrow plan / 1          int4 64-wide lds2 / lds3 (narrow 1: the f16 kernels next to them too)
Not launched by anything: the 64-wide GLU instantiations (compiled, but the launcher never narrows a GLU tile).

After the first exception out of a forward the module touches the device no more: every later case fails at once.

Wall time of the module on an MI355X, 2026-10-20: 8.3 s for its 20 tests -- 1.8 s to create the first engine, 0.6-0.9 s for each
engine's default forwards, 0.01-0.04 s per configuration (three forwards), 0.9 s for the two-context case, 3.3 s for the child
process of the environment route.
"""

import hashlib
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 7
AUDIO_SEED = 29
INPUTS = {"ragged": [1, 33, 129, 257], "one": [1], "tile": [128]}
PLAN = -1   # "chosen from the shape": the switch's default
# (precision, ld, nst, narrow)
CONFIGS = ([(0, 0, n, PLAN) for n in (PLAN, 2, 3, 4)] + [(0, 0, n, 1) for n in (2, 3)] + [(0, 1, PLAN, 1)]
           + [(1, 1, PLAN, 0)] + [(1, 0, n, 0) for n in (2, 3, 4)] + [(1, 0, n, w) for w in (PLAN, 1) for n in (2, 3)])
# layer-0 GEMMs qv_profile_replay_kernel names: (epilogue, N, K)
REPLAY = [("f16_swish", 2048, 512), ("resid", 512, 2048), ("qkv", 1536, 512), ("resid", 512, 512), ("glu", 1024, 512)]

_device_errors = []   # the first exception a forward of this module raised


def expected_name(precision, which, M, ld, nst, narrow):
    """gemm_plan + gemm_kernel restated for the replay shapes of a single-context engine under gemm_tiles(0)"""
    epi, N, K = REPLAY[which]
    if precision == 1 and which == 4:
        return "k_gemm<glu,128>"                      # int8 weights: one kernel whatever is set, and no suffix
    rows = math.ceil(M / 128)
    is_narrow = precision == 1 and (N // 128) * rows < 400
    if narrow >= 0 and epi != "glu":
        is_narrow = bool(narrow)
    bn = 64 if is_narrow else 128
    if ld != 0:
        return f"k_gemm<{epi},{bn}>"
    stages = 2 if (N // bn) * rows >= 400 else 4 if K // 64 >= 16 else 3
    if bn == 64:
        stages = min(stages, 3)
    if 2 <= nst <= (3 if bn == 64 else 4):
        stages = nst
    return f"k_gemm<{epi},{bn},lds{stages}>"


def _audio():
    import forward_ref as FR

    out = {}
    for name, frames in INPUTS.items():
        lens = [FR.samples_for_frames(t) for t in frames]
        out[name] = (FR.clips(lens, AUDIO_SEED).cuda().contiguous(), lens)
    return out


def _forward_words(eng, dev, lens):
    """log-probs of one forward as uint32 words [B, T, 1025] on the host, and T"""
    import torch

    if _device_errors:
        pytest.fail(f"an earlier forward of this module raised ({_device_errors[0]}): the device is not touched again")
    try:
        lp, t = eng.forward(dev, lens)
        torch.cuda.synchronize()
        return lp.cpu().numpy().view(np.uint32).copy(), list(t)
    except BaseException as e:
        _device_errors.append(repr(e))
        raise


def _valid_words(words, t):
    return np.concatenate([words[b, :n].ravel() for b, n in enumerate(t)])


def _assert_same_bits(tag, got, t, ref, t_ref):
    assert t == t_ref, (tag, t, t_ref)
    for b, n in enumerate(t):
        diff = got[b, :n] != ref[b, :n]
        if diff.any():
            total = sum(int(np.count_nonzero(got[u, :m] != ref[u, :m])) for u, m in enumerate(t))
            frame = int(np.flatnonzero(diff.any(axis=1))[0])
            pytest.fail(f"{tag}: {total} words differ from the default pipeline's, first at utterance {b} (T = {n}), frame {frame}")


def _engine(precision, **kw):
    import forward_ref as FR
    import offline_tarteel_amd  # noqa: F401
    from offline_tarteel_amd.engine import Engine

    return Engine(device=0, with_model=True, seed=SEED, precision=precision, max_batch=4, max_samples=FR.samples_for_frames(257), **kw)


@pytest.fixture(scope="module")
def audio():
    return _audio()


@pytest.fixture(scope="module")
def engines(audio):
    """one engine per precision, created on first use, with the default pipeline's words of the three inputs"""
    made = {}

    def get(precision):
        if precision not in made:
            if _device_errors:
                pytest.fail(f"an earlier forward of this module raised ({_device_errors[0]}): the device is not touched again")
            eng = _engine(precision)
            made[precision] = {"eng": eng}
            eng.gemm_tiles(0)
            eng.gemm_pipeline(-1, -1, -1)
            ref, names = {}, {}
            for name, (dev, lens) in audio.items():
                ref[name] = _forward_words(eng, dev, lens)
                names[name] = [eng.replay_kernel(w) for w in range(5)]
            made[precision].update(ref=ref, names=names)
        return made[precision]

    try:
        yield get
    finally:
        for m in made.values():
            m["eng"].gemm_pipeline(-1, -1, -1)
            m["eng"].gemm_tiles(-1)
            m["eng"].close()


@pytest.mark.parametrize("precision", [0, 1])
def test_default_pipeline_is_finite_and_named_as_before(engines, precision):
    """what every case below is compared with: finite over the valid frames (equal NaN patterns would prove nothing), from
    the kernels the defaults have always named"""
    e = engines(precision)
    for name, (words, t) in e["ref"].items():
        assert t == INPUTS[name]
        assert np.isfinite(_valid_words(words, t).view(np.float32)).all(), name
        bn = 64 if precision else 128
        assert e["names"][name] == [f"k_gemm<f16_swish,{bn}>", f"k_gemm<resid,{bn}>", f"k_gemm<qkv,{bn}>", f"k_gemm<resid,{bn}>", "k_gemm<glu,128>"]


@pytest.mark.parametrize("precision,ld,nst,narrow", CONFIGS,
                         ids=[f"p{p}-ld{ld}-nst{'plan' if n < 0 else n}-narrow{'plan' if w < 0 else w}" for p, ld, n, w in CONFIGS])
def test_pipeline_gives_the_default_pipelines_bits(engines, audio, precision, ld, nst, narrow):
    e = engines(precision)
    eng = e["eng"]
    try:
        eng.gemm_pipeline(ld, nst, narrow)
        for name, (dev, lens) in audio.items():
            words, t = _forward_words(eng, dev, lens)
            # 1. the configuration ran: the launcher names the kernels it is meant to reach, and not the default's
            M = sum(INPUTS[name])
            names = [eng.replay_kernel(w) for w in range(5)]
            assert names == [expected_name(precision, w, M, ld, nst, narrow) for w in range(5)], (name, names)
            assert names[0] != e["names"][name][0] and names[1] != e["names"][name][1], (name, names)
            if precision == 1:
                assert names[4] == "k_gemm<glu,128>"          # int8 weights: unaffected, no suffix
            # 2. same bits as the default pipeline
            ref, t_ref = e["ref"][name]
            _assert_same_bits(f"precision {precision}, ld {ld}, nst {nst}, narrow {narrow}, input {name}", words, t, ref, t_ref)
    finally:
        eng.gemm_pipeline(-1, -1, -1)


def test_setter_checks_its_ranges_and_leaves_nothing_behind(engines):
    e = engines(0)
    eng = e["eng"]
    from offline_tarteel_amd.engine import QvError

    try:
        for bad in ((2, -1, -1), (-1, 5, -1), (-1, -1, 2), (-2, -1, -1), (0, 3, 2)):
            with pytest.raises(QvError):
                eng.gemm_pipeline(*bad)
            assert [eng.replay_kernel(w) for w in range(5)] == e["names"]["ragged"], bad   # nothing was set
        eng.gemm_pipeline(0, 3, 1)
        assert eng.replay_kernel(0) == "k_gemm<f16_swish,64,lds3>"
        eng.gemm_pipeline()                                                                      # all three back
        assert eng.replay_kernel(0) == "k_gemm<f16_swish,128>"
    finally:
        eng.gemm_pipeline(-1, -1, -1)


def test_forward_graph_is_keyed_on_the_pipeline(audio):
    """A two-context engine replays a repeating forward as one hipGraph launch.  Changing the pipeline between forwards must
    capture a new graph, never replay the other pipeline's launches; every row predict_batch derives from the log-probs
    (greedy ids of every frame, scores, CTC losses) and the log-probs of a plain forward stay as they were."""
    if _device_errors:
        pytest.fail(f"an earlier forward of this module raised ({_device_errors[0]}): the device is not touched again")
    dev, lens = audio["ragged"]
    eng = _engine(0, contexts=2)
    try:
        assert eng.contexts == 2
        eng.gemm_tiles(0)
        ref_words, t_ref = _forward_words(eng, dev, lens)
        want = None

        def run_until_both_contexts_replay(tag):
            nonlocal want
            replayed = {}
            for i in range(12):                                          # (a context captures a shape the second time it sees it)
                before = eng.forward_graph_stats()["replays"]
                try:
                    res = eng.predict_batch(dev, lens, want_text=True)
                except BaseException as e:
                    _device_errors.append(repr(e))
                    raise
                want = want or res
                assert res == want, (tag, i)
                replayed[int(eng.lib.qv_last_context(eng.h))] = eng.forward_graph_stats()["replays"] == before + 1
                if len(replayed) == 2 and all(replayed.values()):
                    return
            pytest.fail(f"{tag}: no replay on both contexts: {replayed}, {eng.forward_graph_stats()}")

        run_until_both_contexts_replay("default")
        c0 = eng.forward_graph_stats()["captures"]
        assert c0 == 2
        eng.gemm_pipeline(0, 3, -1)
        assert eng.replay_kernel(0) == "k_gemm<f16_swish,128,lds3>"
        run_until_both_contexts_replay("ld 0, nst 3")
        c1 = eng.forward_graph_stats()["captures"]
        assert c1 == c0 + 2, (c0, c1)                                    # one more graph per context
        words, t = _forward_words(eng, dev, lens)
        _assert_same_bits("two contexts, ld 0, nst 3", words, t, ref_words, t_ref)
        eng.gemm_pipeline(-1, -1, -1)                                    # back: the graphs captured under the default are hit again
        run_until_both_contexts_replay("default again")
        assert eng.forward_graph_stats()["captures"] == c1
        assert eng.lib.qv_debug_forward_graph_failures(eng.h) == 0
    finally:
        eng.gemm_pipeline(-1, -1, -1)
        eng.gemm_tiles(-1)
        eng.close()


def test_environment_variables_reach_the_same_kernels(engines, audio):
    """QVERSE_GEMM_LD=0 QVERSE_GEMM_NST=3 QVERSE_GEMM_NARROW=1 in a fresh process (the variables are read once): the same
    kernel names and the same log-prob words of the ragged batch as the setter gives in this process."""
    e = engines(0)
    eng = e["eng"]
    dev, lens = audio["ragged"]
    try:
        eng.gemm_pipeline(0, 3, 1)
        words, t = _forward_words(eng, dev, lens)
        mine = [eng.replay_kernel(0), eng.replay_kernel(1), hashlib.sha256(_valid_words(words, t).tobytes()).hexdigest()]
    finally:
        eng.gemm_pipeline(-1, -1, -1)
    assert mine[:2] == ["k_gemm<f16_swish,64,lds3>", "k_gemm<resid,64,lds3>"]
    root = Path(__file__).resolve().parent.parent
    prog = (
        "import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch, offline_tarteel_amd\n"
        "from offline_tarteel_amd.engine import Engine\n"
        "import forward_ref as FR\n"
        "lens = [FR.samples_for_frames(t) for t in %r]\n"
        "eng = Engine(device=0, with_model=True, seed=%d, precision=0, max_batch=4, max_samples=max(lens))\n"
        "eng.gemm_tiles(0)\n"
        "lp, t = eng.forward(FR.clips(lens, %d).cuda().contiguous(), lens)\n"
        "torch.cuda.synchronize()\n"
        "w = lp.cpu().numpy().view(np.uint32)\n"
        "h = hashlib.sha256(np.concatenate([w[b, :n].ravel() for b, n in enumerate(t)]).tobytes()).hexdigest()\n"
        "print('RESULT', eng.replay_kernel(0), eng.replay_kernel(1), h)\n"
    ) % (str(root), str(root / "tests"), INPUTS["ragged"], SEED, AUDIO_SEED)
    env = {k: v for k, v in os.environ.items() if not k.startswith("QVERSE_GEMM_")}
    env.update(QVERSE_GEMM_LD="0", QVERSE_GEMM_NST="3", QVERSE_GEMM_NARROW="1")
    try:
        p = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300, env=env)
    except subprocess.TimeoutExpired:
        _device_errors.append("the child process of the environment route ran into its time limit")
        raise
    if p.returncode < 0:
        _device_errors.append(f"the child process of the environment route ended by signal {-p.returncode}")
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert line.split()[1:] == mine
