"""The decode stage (csrc/qv_postlogits.hip, k_decode) and the rows behind an utterance's last frame, on the MI355X.

k_decode does the per-frame argmax, the CTC collapse, the piece expansion, the whitespace collapse and strip, the
spaceless copy, the match masks, the word count and the EMPTY / TRUNCATED flags in one kernel.  Here its outputs are read
directly -- the codes the matching kernels consume (Engine.transcript_codes), n_tokens, n_chars, the word count -- and held
to numpy and the oracle on the cases of tests/decode_cases.py (premises: tests/test_decode_host.py), on both matching
windows, alone and in ragged batches.  The second half fills the rows t >= T[b] of a batch with values a kernel must never
look at and asks for every output bit for bit."""

import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import decode_cases as D
from synth import BLANK, synth_logits

pytestmark = pytest.mark.gpu

FLAG_EMPTY, FLAG_TRUNC = 1, 2


@pytest.fixture(scope="module")
def engines():
    from offline_tarteel_amd.engine import Engine

    out = {"default": Engine(device=0, with_model=False, max_batch=16, max_samples=D.MAX_SAMPLES),
           "wide": Engine(device=0, with_model=False, max_batch=16, max_samples=D.MAX_SAMPLES, max_transcript=2048)}
    assert out["default"].max_transcript == 1024 and out["wide"].max_transcript == 2048
    assert out["default"].frames_for(D.MAX_SAMPLES) == D.T_TEXT_MAX
    yield out
    for e in out.values():
        e.close()


@pytest.fixture(params=["default", "wide"])
def eng(request, engines):
    return engines[request.param]


@pytest.fixture(scope="module")
def pc(oracle):
    return D.Pieces(oracle)


@pytest.fixture(scope="module")
def cases(oracle):
    return D.build_cases(oracle)


@pytest.fixture(scope="module")
def refs(oracle, cases):
    """ids / text / codes / words per case, and the oracle's whole answer where the text is non-empty and fits the wide
    window -- computed once, several at a time (a long text costs the oracle seconds, all inside its C library)"""
    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.tables import Tables

    tables = Tables(TABLES_PATH)
    out = {name: D.reference_of(oracle, tables.encode, lp, T) for name, lp, T in cases}
    jobs = [(name, lp) for name, lp, T in cases if 0 < len(out[name]["text"]) <= 2048]
    with ThreadPoolExecutor(max_workers=12) as ex:
        for (name, _), w in zip(jobs, ex.map(lambda j: oracle.predict_logprobs(np.asarray(j[1])), jobs)):
            out[name]["predict"] = w
    return out


def run(eng, group, pad=-50.0, t_max=None):
    """one call of the hot path on a group of cases; per row the result dict with the device's transcript merged in"""
    lp, frames = D.batch_tensor(group, pad, t_max)
    res = eng.decode_retrieve_rerank(torch.from_numpy(lp).cuda().contiguous(), frames)
    tc = eng.transcript_codes(batch=len(group))
    for r, c in zip(res, tc):
        r["codes"], r["q_len"], r["q_words"] = c["codes"].tobytes(), c["n_chars"], c["n_words"]
    return res


def check_against_oracle(got, want, tag):
    """the comparisons and tolerances of check_hot (tests/test_gpu_long_transcript.py); a transcript no verse matches
    (source None) must come back as no prediction"""
    assert got["greedy_ids"] == want["greedy_ids"], tag
    assert got["transcript"] == want["transcript"], tag
    assert (got["surah"], got["ayah"], got["ayah_end"], got["source"]) == (
        want["surah"], want["ayah"], want["ayah_end"], want["source"]), (tag, got, want)
    if want["source"] is None:
        return
    assert got["use_ctc"] == want["use_ctc"], tag
    if want["use_ctc"]:
        assert got["n_candidates"] == want["n_candidates"], tag
    if want["source"] == "text":
        assert got["score"] == want["score_raw"], tag
    else:
        assert abs(got["score"] - want["score_raw"]) <= 1e-3 * max(want["score_raw"], 1e-3), tag


def check_row(eng, pc, name, T, got, ref):
    window = eng.max_transcript
    flags = D.expected_flags(ref, pc, window)
    assert got["greedy_ids"] == ref["ids"], name
    assert got["n_tokens"] == len(ref["ids"]), name
    assert got["t_frames"] == T, name
    assert got["flags"] & (FLAG_EMPTY | FLAG_TRUNC) == flags, (name, got["flags"], flags)
    if flags:
        # an empty or a withheld transcript: no codes, a reported length of 0, no prediction
        assert (got["q_len"], got["n_chars"], got["q_words"], got["codes"]) == (0, 0, 0, b""), name
        assert (got["surah"], got["ayah"], got["ayah_end"], got["source"]) == (0, 0, None, None), name
        return
    assert got["codes"] == ref["codes"].tobytes(), (name, len(got["codes"]), len(ref["codes"]))
    assert got["n_chars"] == got["q_len"] == len(ref["text"]), name
    assert got["q_words"] == ref["words"], name
    assert got["transcript"] == ref["text"], name
    check_against_oracle(got, ref["predict"], name)


def test_decode_stage_against_numpy_and_the_oracle(eng, pc, cases, refs):
    """every case alone: ids, token count, the device's codes byte for byte, lengths, word count, flags, and the whole
    result where there is a transcript to match"""
    seen = set()
    for name, lp, T in cases:
        got = run(eng, [(name, lp, T)])[0]
        check_row(eng, pc, name, T, got, refs[name])
        seen.add(got["flags"] & 3)
    assert seen == {0, FLAG_EMPTY, FLAG_TRUNC}


def test_a_case_alone_equals_its_row_in_a_ragged_batch(eng, pc, cases, refs):
    """... and the same cases sixteen at a time, rows of 0 to 768 frames side by side: field for field what each gave alone"""
    for group in D.batches_of(cases, 16):
        assert len({T for _, _, T in group}) > 4
        batched = run(eng, group)
        for (name, lp, T), got in zip(group, batched):
            check_row(eng, pc, name, T, got, refs[name])
            alone = run(eng, [(name, lp, T)])[0]
            assert got == alone, (name, {k: (got[k], alone[k]) for k in got if got[k] != alone[k]})


def test_transcript_codes_argument_checks(engines):
    """pitch below the window, a batch the context does not hold, a bad context: QV_ERR_ARG (1); above max_batch: QV_ERR_CAPACITY (4)"""
    import ctypes as C

    eng = engines["wide"]
    lp, frames = D.batch_tensor([("x", D.frames_of([5, BLANK, 7], 1), 3)] * 2)
    eng.decode_retrieve_rerank(torch.from_numpy(lp).cuda().contiguous(), frames)
    codes, n, w = np.zeros((17, 2048), np.uint8), np.zeros(17, np.int32), np.zeros(17, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda ctx, batch, pitch: eng.lib.qv_debug_transcript_codes(eng.h, ctx, batch, p(codes), pitch, p(n), p(w))  # noqa: E731
    assert call(0, 2, 2048) == 0 and n[:2].tolist() == [2, 2] and w[:2].tolist() == [1, 1]      # two letters, one word
    assert call(0, 2, 2047) == 1 and call(0, 0, 2048) == 1 and call(1, 2, 2048) == 1 and call(-1, 2, 2048) == 1
    assert call(0, 3, 2048) == 1                  # the context's last batch had two rows
    assert call(0, 17, 2048) == 4
    assert eng.lib.qv_debug_transcript_codes(eng.h, 0, 2, None, 2048, p(n), p(w)) == 1
    eng.debug_retrieve("ا")                       # reuses the workspace: the batch is gone
    assert call(0, 2, 2048) == 1


# ------------------------------------------------------------------ poisoned padding ------------------------------------

T_PAD = 768
PADS = (-50.0, 0.0, float("nan"), float("inf"), 1e30)


@pytest.fixture(scope="module")
def ragged(oracle, cases):
    """ten rows in a [10, 768, 1025] tensor, every one shorter than 766 frames: recitations that pass the gate, corrupted
    ones that fail it, a long recitation clean and corrupted (targets beyond 384 states in the rerank), an empty
    transcript, a one-frame row; and an explicit alignment target for each"""
    def recite(s, a, span, T, seed, rate=0.0, boost=8.0):
        ids = oracle.token_ids(oracle.verse_index(s, a), span).tolist()
        said = ids
        if rate:
            rng = np.random.default_rng(seed)
            said = [int(rng.integers(1, 1024)) if rng.random() < rate else t for t in ids]
        lp = torch.log_softmax(torch.from_numpy(synth_logits(said, T, seed=seed, noise=1.0, boost=boost, rep=2)), -1).numpy()
        return lp, ids

    long_ids = oracle.token_ids(oracle.verse_index(2, 282), 1).tolist()
    rng = np.random.default_rng(35)
    long_bad = [int(rng.integers(1, 1024)) if rng.random() < 0.35 else t for t in long_ids]
    by = {n: lp for n, lp, _ in cases}
    rows = [("112:1", *recite(112, 1, 1, 24, 16)),
            ("1:2", *recite(1, 2, 1, 40, 17)),
            ("36:1-3", *recite(36, 1, 3, 120, 18)),
            ("2:255 30% replaced", *recite(2, 255, 1, 380, 19, rate=0.30)),
            ("67:1-2 40% replaced", *recite(67, 1, 2, 200, 20, rate=0.40)),
            ("2:282", D.frames_of(D.path_of(long_ids) + [BLANK] * 300, 21), long_ids),
            ("2:282 35% replaced", D.frames_of(D.path_of(long_bad) + [BLANK] * 400, 22), long_ids),
            ("blanks only", D.frames_of([BLANK] * 50, 23), [5, 6]),
            ("argmax ties", np.asarray(by["argmax ties"]), [5, 5, 63]),
            ("T=1 token", np.asarray(by["T=1 token"]), [7])]
    group = [(n, lp, lp.shape[0]) for n, lp, _ in rows]
    assert len(group) >= 8 and all(T < 766 for _, _, T in group) and max(T for _, _, T in group) > 384
    targets = [tg[: min(383, (lp.shape[0] - 1) // 2)] if lp.shape[0] > 2 else tg for _, lp, tg in rows]
    base, frames = D.batch_tensor(group, -50.0, T_PAD)
    mask = torch.zeros((len(group), T_PAD, 1), dtype=torch.bool)
    for b, T in enumerate(frames):
        mask[b, T:] = True
    return group, torch.from_numpy(base), frames, mask, targets


def bits(x):
    """a value with every float replaced by its bit pattern and every array by its bytes: == then means bit for bit"""
    if isinstance(x, float):
        return struct.pack("<d", x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    return x


def has_nan(x) -> bool:
    if isinstance(x, float):
        return x != x
    if isinstance(x, np.ndarray):
        if x.dtype.names:
            return any(has_nan(x[n]) for n in x.dtype.names)
        return bool(np.issubdtype(x.dtype, np.floating) and np.isnan(x).any())
    if isinstance(x, dict):
        return any(has_nan(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return any(has_nan(v) for v in x)
    return False


def everything(eng, lp, frames, targets):
    B = len(frames)
    res = eng.decode_retrieve_rerank(lp, frames, align=True, nbest=32)
    codes = eng.transcript_codes(batch=B)
    info, ent = eng.nbest_raw(batch=B, k=32, runners=True)
    al = eng.align(lp, frames, targets)
    return {"results": res, "codes": codes, "nbest_info": info, "nbest_entries": ent, "align": al}


def test_rows_behind_the_last_frame_are_never_read(eng, ragged):
    """the rows t >= T[b] filled with -50, 0, NaN, +inf and 1e30 in turn: the hot path with alignment and n-best, the
    device's transcript, explicit alignment and the n-best records with runners-up all equal the -50 run bit for bit, and
    nothing contains a NaN"""
    from offline_tarteel_amd.engine import FLAG_USED_CTC

    group, base, frames, mask, targets = ragged
    dev, m = base.cuda(), mask.cuda()
    want = None
    for pad in PADS:
        lp = torch.where(m, torch.tensor(pad, dtype=torch.float32, device="cuda"), dev).contiguous()
        got = everything(eng, lp, frames, targets)
        assert not has_nan(got), pad
        if want is None:
            want = bits(got)
            res = got["results"]
            used = [bool(r["flags"] & FLAG_USED_CTC) for r in res]
            assert any(used) and not all(used)                              # gate-fail and gate-pass rows
            assert sum(r["source"] == "ctc" for r in res) >= 2 and sum(r["source"] == "text" and not u for r, u in zip(res, used)) >= 2
            assert any(r["flags"] & FLAG_EMPTY for r in res)                # the empty transcript
            assert sum(a["flags"] == 0 and a["n_tokens"] > 0 for a in got["align"]) >= 8
            assert max(int(e["n_tokens"]) for e in got["nbest_entries"].reshape(-1)) * 2 + 1 > 384
            continue
        g = bits(got)
        for k in want:
            assert g[k] == want[k], (pad, k)
