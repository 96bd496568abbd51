"""Transcription with confidence (csrc/qv_transcribe.hip, k_transcribe; include/qverse.h qv_transcribe /
qv_transcribe_batch) on the MI355X, and the streaming row gated by it.

The reference of every figure is tests/transcribe_ref.py (premises: tests/test_transcribe_host.py): ids, first / last
frames, token log-probs, both float64 averages, the minimum, the blank count and the flag are compared bit for bit on the
cases of tests/decode_cases.py in ragged batches, with hostile padding rows, through the forward, and end to end through
StreamingPipeline with the confidence gate on."""

import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as D
import transcribe_ref as R
from synth import BLANK, VOCAB, synth_audio

pytestmark = pytest.mark.gpu

T_CHUNK = 38            # encoder frames of a 3-s chunk
CHUNK = 48000


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=16, max_samples=D.MAX_SAMPLES)
    assert e.frames_for(CHUNK) == T_CHUNK
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    return D.build_cases(oracle)


@pytest.fixture(scope="module")
def refs(cases):
    return {name: R.transcribe_ref(lp, T) for name, lp, T in cases}


def raw_rows(eng, lp: np.ndarray, frames, pitch=None):
    """one qv_transcribe call; per row the fields in comparable form (floats as their bytes)"""
    info, ids, logp, first, last = eng.transcribe_raw(torch.from_numpy(lp).cuda().contiguous(), frames, pitch)
    out = []
    for b in range(len(frames)):
        n = int(info[b]["n_tokens"])
        out.append({"ids": ids[b, :n].tolist(), "first": first[b, :n].tolist(), "last": last[b, :n].tolist(),
                    "logp": logp[b, :n].tobytes(), "n_tokens": n, "t_frames": int(info[b]["t_frames"]),
                    "n_blank_frames": int(info[b]["n_blank_frames"]), "flags": int(info[b]["flags"]),
                    "min_token_logprob": info[b]["min_token_logprob"].tobytes(), "reserved_f": float(info[b]["reserved_f"]),
                    "avg_logprob": info[b]["avg_logprob"].tobytes(), "frame_avg_logprob": info[b]["frame_avg_logprob"].tobytes(),
                    "tail": (ids[b, n:].tolist(), first[b, n:].tolist(), last[b, n:].tolist(), logp[b, n:].tobytes())})
    return out


def expected(ref: dict) -> dict:
    return {"ids": ref["ids"], "first": ref["first"], "last": ref["last"], "logp": R.bits32(ref["logp"]),
            "n_tokens": ref["n_tokens"], "t_frames": ref["t_frames"], "n_blank_frames": ref["n_blank_frames"],
            "flags": ref["flags"], "min_token_logprob": R.bits32(ref["min_token_logprob"]), "reserved_f": 0.0,
            "avg_logprob": R.bits64(ref["avg_logprob"]), "frame_avg_logprob": R.bits64(ref["frame_avg_logprob"])}


def check(got: dict, ref: dict, tag):
    want = expected(ref)
    for k, v in want.items():
        assert got[k] == v, (tag, k, got[k], v)
    pad = len(got["tail"][0])
    assert got["tail"] == ([-1] * pad, [-1] * pad, [-1] * pad, np.zeros(pad, np.float32).tobytes()), tag


def test_decode_cases_in_ragged_batches(eng, cases, refs):
    """T = 0, 1, 768, every tie frame, the -inf rows, runs across frames 63|64 and 127|128: every output bit for bit"""
    seen = set()
    for group in D.batches_of(cases, 16):
        lp, frames = D.batch_tensor(group)
        for (name, _, T), got in zip(group, raw_rows(eng, lp, frames)):
            check(got, refs[name], name)
            seen.add(name)
    assert {"T=0", "T=1 token", "T=1 blank", "T=768", "argmax ties", "-inf everywhere", "-inf but one",
            "merge across 63|64 and 127|128"} <= seen
    r = refs["-inf everywhere"]
    assert r["ids"] == [0] and np.isneginf(r["logp"][0])
    assert any(b - a >= 2 and a <= 63 < b for a, b in zip(refs["merge across 63|64 and 127|128"]["first"],
                                                         refs["merge across 63|64 and 127|128"]["last"]))


def test_padding_rows_are_never_read(eng, cases, refs):
    """the rows t >= T[b] hold NaN and the tensor is longer than its longest row: nothing changes"""
    longer = 0
    for group in D.batches_of(cases, 16):
        t_long = max(T for _, _, T in group)
        t_max = min(D.T_FULL, t_long + 5)
        longer += t_max > t_long
        lp, frames = D.batch_tensor(group, pad=float("nan"), t_max=t_max)
        assert lp.shape[1] == t_max and np.isnan(lp[0, frames[0]:]).all()
        for (name, _, T), got in zip(group, raw_rows(eng, lp, frames)):
            check(got, refs[name], name)
    assert longer >= 1


def test_pitch_above_t_max_and_null_optional_arrays(eng, cases, refs):
    group = [c for c in cases if c[0] in ("65 tokens", "T=0", "argmax ties", "-inf everywhere")]
    assert len(group) == 4
    lp, frames = D.batch_tensor(group)
    t_max = lp.shape[1]
    for (name, _, T), got in zip(group, raw_rows(eng, lp, frames, pitch=t_max + 7)):
        assert len(got["tail"][0]) == t_max + 7 - refs[name]["n_tokens"]
        check(got, refs[name], name)
    dev = torch.from_numpy(lp).cuda().contiguous()
    from offline_tarteel_amd.engine import TRANSCRIPT_INFO_DTYPE

    info = np.zeros(4, TRANSCRIPT_INFO_DTYPE)
    ids = np.full((4, t_max), 7, np.int32)
    t = np.asarray(frames, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = eng.lib.qv_transcribe(eng.h, C.c_void_p(dev.data_ptr()), p(t), 4, t_max, p(info), p(ids), None, None, None, t_max, None)
    assert rc == 0
    for b, (name, _, T) in enumerate(group):
        n = refs[name]["n_tokens"]
        assert int(info[b]["n_tokens"]) == n and ids[b, :n].tolist() == refs[name]["ids"] and (ids[b, n:] == -1).all(), name
        assert info[b]["avg_logprob"].tobytes() == R.bits64(refs[name]["avg_logprob"]), name


def test_ids_equal_the_decode_stage(eng, cases):
    """k_transcribe and k_decode collapse the same tensors to the same ids"""
    for group in D.batches_of(cases, 16):
        lp, frames = D.batch_tensor(group)
        dev = torch.from_numpy(lp).cuda().contiguous()
        dec = eng.decode_retrieve_rerank(dev, frames, want_text=True)
        tr = eng.transcribe_logprobs(dev, frames)
        for (name, _, T), a, b in zip(group, dec, tr):
            assert a["greedy_ids"] == [k["id"] for k in b["tokens"]], name
            assert a["transcript"] == b["text"], name
            assert b["n_tokens"] == len(b["tokens"]) and b["t_frames"] == T, name
            assert all(k["first"] <= k["last"] for k in b["tokens"]), name


def test_error_paths(eng):
    from offline_tarteel_amd.engine import TRANSCRIPT_INFO_DTYPE

    lib, p = eng.lib, (lambda a: a.ctypes.data_as(C.c_void_p))
    dev = torch.zeros((1, 4, VOCAB), dtype=torch.float32, device="cuda")
    lp = C.c_void_p(dev.data_ptr())
    info = np.zeros(17, TRANSCRIPT_INFO_DTYPE)
    info["n_tokens"] = -77
    ids = np.full((17, 1024), 5, np.int32)
    t = np.full(17, 4, np.int32)
    ERR_ARG, ERR_CAPACITY, ERR_NO_MODEL = 1, 4, 5
    assert lib.qv_transcribe(eng.h, lp, p(t), 1, 4, None, p(ids), None, None, None, 4, None) == ERR_ARG          # null info
    assert lib.qv_transcribe(eng.h, lp, p(t), 1, 4, p(info), None, None, None, None, 4, None) == ERR_ARG         # null ids
    assert lib.qv_transcribe(eng.h, lp, p(t), 0, 4, p(info), p(ids), None, None, None, 4, None) == ERR_ARG       # batch = 0
    assert lib.qv_transcribe(eng.h, lp, p(t), 1, 4, p(info), p(ids), None, None, None, 3, None) == ERR_ARG       # pitch < t_max
    assert lib.qv_transcribe(eng.h, lp, p(t), 17, 4, p(info), p(ids), None, None, None, 4, None) == ERR_CAPACITY  # batch > max_batch
    assert lib.qv_transcribe(eng.h, lp, p(t), 1, D.T_FULL + 1, p(info), p(ids), None, None, None, 1024, None) == ERR_CAPACITY
    audio = torch.zeros((1, 16000), dtype=torch.float32, device="cuda")
    ln = np.array([16000], np.int64)
    assert lib.qv_transcribe_batch(eng.h, C.c_void_p(audio.data_ptr()), p(ln), 1, 16000, p(info), p(ids), None, None, None, 1024,
                                   None) == ERR_NO_MODEL
    assert b"model" in lib.qv_last_error(eng.h)
    # nothing ran: the output arrays are as they were
    assert (info["n_tokens"] == -77).all() and (ids == 5).all()


def test_forward_path_equals_the_restatement_on_the_forwards_log_probs():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=11, max_batch=4, max_samples=CHUNK)
    try:
        lengths = [16000, 27200, CHUNK]
        host = synth_audio(3, CHUNK)
        for b, n in enumerate(lengths):
            host[b, n:] = 0.0
        audio = torch.from_numpy(np.ascontiguousarray(host, np.float32)).cuda()
        lp, T = e.forward(audio, lengths)
        assert T == [e.frames_for(n) for n in lengths] and T[2] == T_CHUNK
        lp = lp.cpu().numpy()
        got = e.transcribe_batch(audio, lengths, confidence=True)
        plain = e.transcribe_batch(audio, lengths)
        for b in range(3):
            ref, g = R.transcribe_ref(lp[b], T[b]), got[b]
            assert [k["id"] for k in g["tokens"]] == ref["ids"], b
            assert [k["first"] for k in g["tokens"]] == ref["first"] and [k["last"] for k in g["tokens"]] == ref["last"], b
            assert R.bits32([k["logp"] for k in g["tokens"]]) == R.bits32(ref["logp"]), b
            assert R.bits64(g["avg_logprob"]) == R.bits64(ref["avg_logprob"]), b
            assert R.bits64(g["frame_avg_logprob"]) == R.bits64(ref["frame_avg_logprob"]), b
            assert R.bits32(g["min_token_logprob"]) == R.bits32(ref["min_token_logprob"]), b
            assert (g["n_tokens"], g["t_frames"], g["n_blank_frames"], g["flags"]) == (
                ref["n_tokens"], T[b], ref["n_blank_frames"], ref["flags"]), b
            assert g["text"] == plain[b] == e.transcript_of(ref["ids"]), b
    finally:
        e.close()


# ------------------------------------------------------------------ the gate, end to end ---------------------------------

def confident_chunk(ids, seed):
    path = D.path_of(ids)
    assert len(path) <= T_CHUNK
    return D.frames_of(path + [BLANK] * (T_CHUNK - len(path)), seed)


def low_chunk(ids, seed):
    """literal frames: every entry clearly negative, the intended id at -1.5"""
    path = D.path_of(ids)
    path = path + [BLANK] * (T_CHUNK - len(path))
    lp = np.stack([D.base_frame(seed + t) for t in range(T_CHUNK)])
    lp[np.arange(T_CHUNK), path] = np.float32(-1.5)
    return np.ascontiguousarray(lp, np.float32)


class ServedEngine:
    """the engine, with transcribe_batch answering from prepared chunk log-probs (in chunk order) through the real
    qv_transcribe; everything else is the engine's"""

    def __init__(self, eng, chunks):
        self._eng, self._chunks, self._at = eng, chunks, 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def transcribe_batch(self, audio, lengths, confidence=False):
        n = len(lengths)
        assert all(int(x) == CHUNK for x in lengths)
        part = self._chunks[self._at: self._at + n]
        self._at += n
        assert len(part) == n
        out = self._eng.transcribe_logprobs(torch.from_numpy(np.stack(part)).cuda().contiguous(), [T_CHUNK] * n)
        return out if confidence else [d["text"] for d in out]


def test_streaming_gate_end_to_end(eng, oracle, monkeypatch):
    from offline_tarteel_amd.streaming import MIN_CHUNK_LOG_PROB, StreamingPipeline

    def ids_of(s, a):
        return oracle.token_ids(oracle.verse_index(s, a), 1).tolist()

    G, L = confident_chunk, low_chunk
    # recording 1: good, three low-confidence chunks (whole verses: fed to the tracker they would be emitted), good
    rec1 = [G(ids_of(112, 1), 900), L(ids_of(112, 2), 910), L(ids_of(112, 3), 920), L(ids_of(112, 4), 930), G(ids_of(113, 1), 940)]
    # recording 2: a weak match, a verse that displaces it (the weak one becomes a tentative emission), TWO low chunks, good
    weak = ids_of(113, 1)[:2] + ids_of(113, 2)[-2:]     # "bsm" + "ma khalaq": three words no verse matches well
    rec2 = [G(weak, 950), G(ids_of(113, 1), 960), L(ids_of(114, 1), 970), L(ids_of(114, 1), 980), G(ids_of(112, 1), 990)]
    rec2_three = rec2[:4] + [L(ids_of(114, 1), 985)] + rec2[4:]
    low = {(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)}

    def dicts(chunks):
        out = []
        for lp in chunks:
            r = R.transcribe_ref(lp, T_CHUNK)
            out.append({"text": eng.transcript_of(r["ids"]), "avg_logprob": float(r["avg_logprob"]), "ids": r["ids"]})
        return out

    want = [dicts(rec1), dicts(rec2)]
    for i, rec in enumerate(want):
        for k, d in enumerate(rec):
            # the premises, from the restatement: low chunks are below the gate with their ids intact, the others above it
            assert (d["avg_logprob"] < MIN_CHUNK_LOG_PROB) == ((i, k) in low), (i, k, d["avg_logprob"])
            assert len(d["text"].split()) >= 2, (i, k)
    assert want[0][1]["ids"] == ids_of(112, 2) and want[1][2]["ids"] == ids_of(114, 1)
    assert abs(want[0][1]["avg_logprob"] + 1.5) < 1e-6

    pipe = StreamingPipeline(eng)

    def scripted(rec):
        calls = []

        def fn(path):
            calls.append(path)
            d = rec[len(calls) - 1]
            return {"text": d["text"], "avg_logprob": d["avg_logprob"]}

        out = pipe.run_on_audio_chunked(np.zeros(CHUNK * len(rec), np.float32), fn, chunk_seconds=3.0)
        assert len(calls) == len(rec)
        return out

    reference = [scripted(want[0]), scripted(want[1])]
    # the second script does hold a tentative emission across its two low chunks: a third low chunk retracts it
    assert scripted(dicts(rec2_three)) != reference[1]
    assert any(e["score"] < 0.7 for e in reference[1][:-1])

    recordings = [np.zeros(CHUNK * 5, np.float32), np.zeros(CHUNK * 5, np.float32)]
    gated = StreamingPipeline(ServedEngine(eng, rec1 + rec2)).run_on_audio_chunked_batch(recordings, confidence_gate=True)
    assert gated == reference
    ungated = StreamingPipeline(ServedEngine(eng, rec1 + rec2)).run_on_audio_chunked_batch(recordings, confidence_gate=False)
    assert ungated[0] != gated[0]
    assert len(ungated[0]) > len(gated[0])     # the three low chunks were fed to the tracker
    # None reads the environment; the default is off
    monkeypatch.delenv("QVERSE_STREAM_GATE", raising=False)
    assert StreamingPipeline(ServedEngine(eng, rec1 + rec2)).run_on_audio_chunked_batch(recordings) == ungated
    monkeypatch.setenv("QVERSE_STREAM_GATE", "1")
    assert StreamingPipeline(ServedEngine(eng, rec1 + rec2)).run_on_audio_chunked_batch(recordings) == gated
