"""The entry points that run the forward (csrc/qv_capi.hip) share their opening -- model present, capacity, the context and
batch of a *_results_ctx call -- and their handling of batches in flight.  Two things are pinned here.

Refusals keep their code and text: every call of the first half is refused before any launch, through the C ABI itself (the
Python wrappers assert first), and the expected (rc, text) are literals.

Batches in flight: a call that runs the forward on the caller's stream while both contexts of an engine are busy waits for
them, returns what it returns on an idle engine, leaves the earlier batches' results alone and ends the alignment of the
context whose log-probs it overwrote."""
import ctypes as C

import numpy as np
import pytest
import torch

from synth import synth_audio

pytestmark = pytest.mark.gpu

NO_MODEL = (5, "engine created without a model (with_model = 0)")
LENS = [32000, 24000]


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def dev(t):
    return C.c_void_p(t.data_ptr())


def outcome(e, rc):
    return rc, e.lib.qv_last_error(e.h).decode()


@pytest.fixture(scope="module")
def bare():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=2, max_samples=32000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=32000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def clips():
    """two batches of two clips of 32,000 and 24,000 samples"""
    out = []
    for seed in (20260630, 1):
        a = torch.from_numpy(synth_audio(2, 32000, seed=seed)).cuda()
        a[1, 24000:] = 0
        out.append(a.contiguous())
    return out


class Buffers:
    """host outputs large enough for every call below at up to three rows"""

    def __init__(self, e):
        self.info = np.zeros((3, 16), np.int64)            # 128 bytes per row: above every *_info struct
        self.ent = np.zeros((3, 64, 72), np.uint8)         # above [k] of every *_entry struct
        self.i32 = [np.zeros((3, 512), np.int32) for _ in range(3)]
        self.i16 = [np.zeros((3, 512), np.int16) for _ in range(2)]
        self.u16 = np.zeros((3, 512), np.uint16)
        self.f32 = np.zeros((3, 512), np.float32)
        self.ops = np.zeros((3, 1280 + e.max_transcript), np.uint8)
        self.words = np.zeros((3, 288, 12), np.uint8)
        self.codes = np.zeros((3, e.max_transcript), np.uint8)
        self.targets, self.tlens = np.zeros(8, np.uint16), np.ones(3, np.int32)


def batch_calls(e, audio, ln, batch, n_max, info=True):
    """the three forward-then-decode entry points with everything valid but what the arguments say"""
    b, s, ln = Buffers(e), e._stream(), np.ascontiguousarray(np.asarray(ln, np.int64))
    inf = ptr(b.info) if info else None
    lib, a = e.lib, dev(audio)
    return {
        "qv_transcribe_batch": lambda: lib.qv_transcribe_batch(e.h, a, ptr(ln), batch, n_max, inf, ptr(b.i32[0]), ptr(b.f32), ptr(b.i16[0]),
                                                               ptr(b.i16[1]), 512, s),
        "qv_beam_batch": lambda: lib.qv_beam_batch(e.h, a, ptr(ln), batch, n_max, 3, 8, 5, inf, ptr(b.ent), ptr(b.i32[0]), 512, s),
        "qv_scan_batch": lambda: lib.qv_scan_batch(e.h, a, ptr(ln), batch, n_max, 6, 0.5, 5, None, inf, ptr(b.ent), None, s),
    }


def test_no_model(bare, clips):
    e, audio, b, s = bare, clips[0], Buffers(bare), bare._stream()
    ln = np.asarray(LENS, np.int64)
    lp = torch.empty((2, 26, 1025), dtype=torch.float32, device="cuda")
    calls = dict(batch_calls(e, audio, ln, 2, 32000))
    calls["qv_forward"] = lambda: e.lib.qv_forward(e.h, dev(audio), ptr(ln), 2, 32000, dev(lp), 26, ptr(b.i32[0]), s)
    calls["qv_predict_batch_async"] = lambda: e.lib.qv_predict_batch_async(e.h, dev(audio), ptr(ln), 2, 32000, s)
    calls["qv_transcribe_long"] = lambda: e.lib.qv_transcribe_long(e.h, dev(audio), 32000, ptr(ln), 2, 0, -1, ptr(b.info), ptr(b.i32[0]),
                                                                   ptr(b.f32), ptr(b.i32[1]), ptr(b.i32[2]), 512, s)
    calls["qv_align_long"] = lambda: e.lib.qv_align_long(e.h, dev(audio), 32000, ptr(ln), 2, 0, -1, ptr(b.targets), ptr(b.tlens), ptr(b.info),
                                                         ptr(b.i32[0]), ptr(b.i32[1]), ptr(b.f32), 512, s)
    assert len(calls) == 7
    for name, call in calls.items():
        assert outcome(e, call()) == NO_MODEL, name


def test_batch_over_capacity(model):
    e = model
    audio = torch.zeros((3, 32000), dtype=torch.float32, device="cuda")
    ln = np.full(3, 32000, np.int64)
    for name, call in batch_calls(e, audio, ln, 3, 32000).items():
        assert outcome(e, call()) == (4, name + ": batch exceeds engine capacity"), name
    rc = e.lib.qv_predict_batch_async(e.h, dev(audio), ptr(ln), 3, 32000, e._stream())
    assert outcome(e, rc) == (4, "batch exceeds engine capacity")


def test_audio_over_capacity(model):
    e = model
    audio = torch.zeros((1, 48000), dtype=torch.float32, device="cuda")
    ln = np.full(1, 48000, np.int64)
    for name, call in batch_calls(e, audio, ln, 1, 48000).items():
        assert outcome(e, call()) == (4, name + ": audio longer than engine capacity"), name
    rc = e.lib.qv_predict_batch_async(e.h, dev(audio), ptr(ln), 1, 48000, e._stream())
    assert outcome(e, rc) == (4, "audio longer than engine capacity")


def test_null_info_host(model, clips):
    want = {
        "qv_transcribe_batch": "qv_transcribe_batch: null argument or empty batch",
        "qv_beam_batch": "qv_beam_batch: null argument, empty batch, max_span outside 1..6, beam outside 1..QV_BEAM_MAX, "
                         "k outside 1..beam or pitch < t_max",
        "qv_scan_batch": "qv_scan_batch: null argument, empty batch, max_span outside 1..6, k outside 1..QV_SCAN_MAX or "
                         "a surah mask that selects nothing",
    }
    for name, call in batch_calls(model, clips[0], LENS, 2, 32000, info=False).items():
        assert outcome(model, call()) == (1, want[name]), name


def test_bad_context_or_batch(model):
    e, b = model, Buffers(model)
    n_ctx = int(e.lib.qv_context_count(e.h))
    assert n_ctx == 1
    calls = {
        "qv_align_results_ctx": (lambda k, n: e.lib.qv_align_results_ctx(e.h, k, n, ptr(b.info), ptr(b.u16), ptr(b.i16[0]), ptr(b.i16[1]),
                                                                         ptr(b.f32), 512),
                                 "bad context, null argument, empty batch or pitch < QV_ALIGN_MAX_TOKENS"),
        "qv_nbest_results_ctx": (lambda k, n: e.lib.qv_nbest_results_ctx(e.h, k, n, 5, 0, ptr(b.info), ptr(b.ent)),
                                 "bad context, null argument, empty batch, k outside 1..QV_NBEST_MAX or unknown flags"),
        "qv_correct_results_ctx": (lambda k, n: e.lib.qv_correct_results_ctx(e.h, k, n, 0, ptr(b.info), ptr(b.ops), b.ops.shape[1],
                                                                             ptr(b.words), 288),
                                   "bad context, null argument, empty batch, unknown flags or a pitch below its cap"),
        "qv_debug_transcript_codes": (lambda k, n: e.lib.qv_debug_transcript_codes(e.h, k, n, ptr(b.codes), b.codes.shape[1], ptr(b.i32[0]),
                                                                                   ptr(b.i32[1])),
                                      "bad context, null argument, empty batch or pitch < qv_max_transcript"),
    }
    for name, (call, rule) in calls.items():
        assert outcome(e, call(n_ctx, 2)) == (1, f"{name}: {rule}"), name
        assert outcome(e, call(0, 3)) == (4, f"{name}: batch exceeds engine capacity"), name


# ---------------------------------------------------------------- batches in flight ----
def raw_calls(e, audio, lens):
    """qv_transcribe_batch, qv_beam_batch(beam 8, k 5) and qv_scan_batch(k 5) as the wrappers call them: the bytes of every array"""
    from offline_tarteel_amd.engine import (BEAM_ENTRY_DTYPE, BEAM_INFO_DTYPE, SCAN_ENTRY_DTYPE, SCAN_INFO_DTYPE,
                                             TRANSCRIPT_INFO_DTYPE)

    B, N = audio.shape
    ln = np.ascontiguousarray(np.asarray(lens, np.int64))
    pitch, s = e.frames_for(int(ln.max())), e._stream()
    out = {}
    t = [np.zeros(B, TRANSCRIPT_INFO_DTYPE), np.zeros((B, pitch), np.int32), np.zeros((B, pitch), np.float32),
         np.zeros((B, pitch), np.int16), np.zeros((B, pitch), np.int16)]
    assert e.lib.qv_transcribe_batch(e.h, dev(audio), ptr(ln), B, N, *map(ptr, t), pitch, s) == 0
    out["transcribe"] = t
    bm = [np.zeros(B, BEAM_INFO_DTYPE), np.zeros((B, 5), BEAM_ENTRY_DTYPE), np.full((B, pitch), -1, np.int32)]
    assert e.lib.qv_beam_batch(e.h, dev(audio), ptr(ln), B, N, 3, 8, 5, *map(ptr, bm), pitch, s) == 0
    out["beam"] = bm
    sc = [np.zeros(B, SCAN_INFO_DTYPE), np.zeros((B, 5), SCAN_ENTRY_DTYPE)]
    assert e.lib.qv_scan_batch(e.h, dev(audio), ptr(ln), B, N, 6, float(e.cfg.span_penalty), 5, None, *map(ptr, sc), None, s) == 0
    out["scan"] = sc
    return {k: [a.tobytes() for a in v] for k, v in out.items()}


def test_forward_calls_with_both_contexts_busy(model, clips):
    from offline_tarteel_amd.engine import Engine, QvError

    t_max = model.frames_for(32000)
    want = [model.predict_batch(a, LENS) for a in clips]
    e = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=32000, contexts=2)
    try:
        assert e.contexts == 2
        ctx = [e.predict_batch_async(a, LENS) for a in clips]
        assert sorted(ctx) == [0, 1]
        busy = raw_calls(e, clips[0], LENS)            # both contexts in flight: no wait in between
        for k in ctx:
            e.wait(k)
        idle = raw_calls(e, clips[0], LENS)
        assert busy == idle
        assert any(busy["transcribe"][0]) and any(busy["beam"][0]) and any(busy["scan"][0])   # (the info records were written)
        for k, w in zip(ctx, want):
            assert e.fetch_results(k, 2, t_max, want_text=True) == w
        # the last context's log-probs were overwritten by those forwards: its batch can no longer be aligned (the other's can)
        with pytest.raises(QvError, match="holds no batch"):
            e.align_results(ctx=ctx[-1], batch=2)
        assert len(e.align_results(ctx=ctx[0], batch=2)) == 2
    finally:
        e.close()


# ---------------------------------------------------------------- the ingest entry points ----
def test_resampler_and_mixdown_refusals(bare):
    """qv_upfirdn, qv_upfirdn_batch and qv_mixdown_batch refuse a bad argument with QV_ERR_ARG before any launch -- every
    buffer here is large enough for what the refused call names, a refused negative source row included -- and the valid
    call after each refusal returns the bytes it returned before the first."""
    from offline_tarteel_amd.audio import resample_plan

    e, lib, s = bare, bare.lib, bare._stream()
    R, N, ARG = 1025, 64, 1
    x = torch.from_numpy((np.random.default_rng(5).standard_normal((R + 1, N)) * 0.3).astype(np.float32)).cuda()
    x1 = C.c_void_p(x.data_ptr() + N * 4)                  # row 1 of x: R rows behind it, one in front
    up, down, taps, m0, n_out = resample_plan(9, 10, N)
    assert (up, down, n_out) == (9, 10, 58)
    y1, yb, ym = (torch.zeros((R, N), dtype=torch.float32, device="cuda") for _ in range(3))
    lens, frames, src = np.full(R, N, np.int64), np.full(R, N // 2, np.int64), np.arange(R, dtype=np.int32)

    def single(**k):
        a = dict(e=e.h, x=x1, n_in=N, taps=ptr(taps), n_taps=len(taps), up=up, down=down, m0=m0, n_out=n_out, y=dev(y1))
        a.update(k)
        return lib.qv_upfirdn(a["e"], a["x"], a["n_in"], a["taps"], a["n_taps"], a["up"], a["down"], a["m0"], a["n_out"], a["y"], s)

    def batch(**k):
        a = dict(e=e.h, x=x1, x_pitch=N, src=ptr(src), lens=ptr(lens), rows=3, taps=ptr(taps), n_taps=len(taps), up=up, down=down,
                 m0=m0, y=dev(yb), y_pitch=N)
        a.update(k)
        return lib.qv_upfirdn_batch(a["e"], a["x"], a["x_pitch"], a["src"], a["lens"], a["rows"], a["taps"], a["n_taps"], a["up"],
                                    a["down"], a["m0"], a["y"], a["y_pitch"], s)

    def mix(**k):
        a = dict(e=e.h, x=x1, x_pitch=N, frames=ptr(frames), rows=3, channels=2, y=dev(ym), y_pitch=N)
        a.update(k)
        return lib.qv_mixdown_batch(a["e"], a["x"], a["x_pitch"], a["frames"], a["rows"], a["channels"], a["y"], a["y_pitch"], s)

    def valid():
        assert (single(), batch(), mix()) == (0, 0, 0)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (y1, yb, ym)]

    want = valid()
    assert any(want[0]) and any(want[1]) and any(want[2])
    long_row, neg_src, neg_frames, wide_frames = lens.copy(), src.copy(), frames.copy(), frames.copy()
    long_row[1], neg_src[2], neg_frames[1], wide_frames[0] = N + 1, -1, -1, N // 2 + 1
    refused = {
        "qv_upfirdn": (single, [dict(e=None), dict(x=None), dict(taps=None), dict(y=None), dict(n_in=0), dict(n_taps=0), dict(up=0),
                                dict(down=0), dict(m0=-1), dict(n_out=-1)]),
        "qv_upfirdn_batch": (batch, [dict(e=None), dict(x=None), dict(lens=None), dict(taps=None), dict(y=None), dict(rows=0),
                                     dict(rows=R), dict(n_taps=0), dict(up=0), dict(down=0), dict(m0=-1), dict(x_pitch=0),
                                     dict(y_pitch=0), dict(lens=ptr(long_row)), dict(y_pitch=n_out - 1), dict(src=ptr(neg_src))]),
        "qv_mixdown_batch": (mix, [dict(e=None), dict(x=None), dict(frames=None), dict(y=None), dict(rows=0), dict(rows=R),
                                   dict(channels=0), dict(channels=65), dict(frames=ptr(neg_frames)), dict(frames=ptr(wide_frames)),
                                   dict(y_pitch=N // 2 - 1)]),
    }
    text = {"lens": "qv_upfirdn_batch: a row's length is outside [1, x_pitch]", "y_pitch": "qv_upfirdn_batch: y_pitch is shorter than a row's output"}
    for name, (call, cases) in refused.items():
        for k in cases:
            assert call(**k) == ARG, (name, list(k))
            key = next(iter(k))
            if name == "qv_upfirdn_batch" and key in text and k[key]:
                assert e.lib.qv_last_error(e.h).decode() == text[key], (name, key)
            assert valid() == want, (name, list(k))
    # the largest table a call takes is taken: 1,024 rows
    assert batch(rows=R - 1) == 0 and mix(rows=R - 1) == 0
    torch.cuda.synchronize()
    assert yb.cpu().numpy()[:3].tobytes() == np.frombuffer(want[1], np.float32).reshape(R, N)[:3].tobytes()
