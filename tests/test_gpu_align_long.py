"""Word and verse timings for recordings of any length (csrc/qv_align_long.hip: k_long_keep, k_align_long; include/qverse.h
qv_align_windows / qv_align_long) on the MI355X, against the numpy restatement (tests/align_long_ref.py over
tests/long_ref.py's ownership).

Paths (first, last) and flags must be EQUAL and the path score bit-equal (one float32 add per state and frame on both
sides); the per-token mean log-prob is held to the project's own bound, n_frames * 2**-23 relative (tests/align_ref.py).
How close windowed log-probs come to ONE forward over the whole recording is not a subject of these tests.

The engines are small, as in tests/test_gpu_long_audio.py: max_samples = 48,000 (windows of 37 frames = 47,360 samples, 38
frames each) and max_batch = 4; one engine of the largest capacity (979,200 samples: windows of 765 frames, 766 frames
each; qv_align's 768 rows) serves the comparison with qv_align and the longest target."""

import ctypes as C

import numpy as np
import pytest
import torch

import align_long_ref as A
import align_ref
import decode_cases as D
import long_ref as L
from synth import BLANK, frame_path, synth_audio

pytestmark = pytest.mark.gpu

MAX_SAMPLES = 48000
KW = 37
WINDOW = KW * L.HOP
BIG_SAMPLES = 979200
ERR_ARG, ERR_CAPACITY, ERR_NO_MODEL = 1, 4, 5


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=4, max_samples=MAX_SAMPLES)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=11, max_batch=4, max_samples=MAX_SAMPLES)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=16, max_samples=BIG_SAMPLES)
    yield e
    e.close()


def samples_for(T: int) -> int:
    return (T - 1) * L.HOP + 640


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def check_row(info, first, last, logp, want, ids, T, n_windows, tag):
    """one row of the raw arrays against a reference result, the padding behind the tokens included"""
    n = len(ids)
    assert int(info["flags"]) == want["flags"], (tag, int(info["flags"]), want["flags"])
    assert (int(info["n_tokens"]), int(info["t_frames"]), int(info["n_windows"]), float(info["reserved_f"])) == (n, T, n_windows, 0.0), tag
    if want["flags"]:
        assert (first == -1).all() and (last == -1).all() and not logp.any() and float(info["score"]) == 0.0, tag
        return
    assert bits(info["score"]) == bits(want["score"]), (tag, float(info["score"]), float(want["score"]))
    assert np.array_equal(first[:n], want["first"]) and np.array_equal(last[:n], want["last"]), tag
    frames = (want["last"] - want["first"] + 1).astype(np.float64)
    err = np.abs(logp[:n].astype(np.float64) - want["logp"].astype(np.float64))
    print(tag, "logp: largest error / bound", float((err / (frames * 2.0 ** -23 * np.abs(want["logp"]))).max()))
    assert (err <= frames * 2.0 ** -23 * np.abs(want["logp"].astype(np.float64))).all(), (tag, float(err.max()))
    assert (first[n:] == -1).all() and (last[n:] == -1).all() and not logp[n:].any(), tag


def straddles(want, plan) -> int:
    """tokens whose [first, last] holds frames of two windows"""
    seams = np.array([plan.lo(w) for w in range(1, plan.n_windows)])
    return int(((want["first"][:, None] < seams[None, :]) & (seams[None, :] <= want["last"][:, None])).any(axis=1).sum())


# ------------------------------------------------------------------ 1. the windows API against the reference --------------

def planted_recording(T: int, seed: int):
    """(ids, log-probs [T, 1025]): tokens four frames long with a blank behind each (tokens 2 and 3 equal)"""
    n = (T - 2) // 5
    ids = ((np.arange(n) * 37 + 11 + seed) % 1024).astype(np.int64)
    if n > 4:
        ids[3] = ids[2]
    return ids, D.frames_of(frame_path(ids, T, rep=4), 6000 + seed)


@pytest.fixture(scope="module")
def window_cases():
    """{margin: [(n, plan, ids, lp, ref)]}: three ragged recordings per margin -- 200 frames, one window, 193 frames"""
    out = {}
    for margin in (0, 6, 18):
        recs = []
        for k, T in enumerate((200, 38, 193)):
            n = WINDOW if T == 38 else samples_for(T)
            plan = L.plan(n, MAX_SAMPLES, WINDOW, margin)
            assert plan.t_total == T and (plan.n_windows == 1) == (T == 38)
            ids, lp = planted_recording(T, 10 * margin + k)
            ref = A.viterbi(lp, ids)
            assert ref["flags"] == 0
            if plan.n_windows > 1:   # the premise: a token's frames lie in two windows
                assert straddles(ref, plan) >= 1, (margin, T)
            recs.append((n, plan, ids, lp, ref))
        out[margin] = recs
    assert out[6][0][1].n_windows == 8 and out[0][0][1].n_windows == 6 and out[18][0][1].n_windows == 164   # > 4 windows: several rounds
    return out


@pytest.mark.parametrize("hole", ["nan", "poison"])
@pytest.mark.parametrize("margin", [0, 6, 18])
@pytest.mark.parametrize("rows", [1, 3])
def test_windows_api_against_the_reference(eng, window_cases, margin, rows, hole):
    recs = window_cases[margin][:rows]
    t_max = KW + 1 + (3 if rows == 3 else 0)           # the tensor may be longer than a window
    cut_of = (lambda lp, plan, ids: L.cut_logprobs(lp, plan, t_max)) if hole == "nan" else (lambda lp, plan, ids: A.poisoned(lp, plan, t_max, ids))
    parts = [cut_of(lp, plan, ids) for _, plan, ids, lp, _ in recs]
    for part, (_, plan, ids, lp, ref) in zip(parts, recs):   # what the reference saw is what the ownership rule leaves of the windows
        assert np.array_equal(A.stitched(part, plan), lp)
    cut = np.concatenate(parts)
    assert (np.isnan(cut).any() if hole == "nan" else (cut == 100.0).any()) and cut.shape[0] == sum(r[1].n_windows for r in recs)
    dev = torch.from_numpy(cut).cuda().contiguous()
    pitch = max(len(r[2]) for r in recs) + (5 if rows == 3 else 0)
    info, first, last, logp = eng.align_windows_raw(dev, [r[0] for r in recs], [r[2] for r in recs], WINDOW, margin, pitch=pitch)
    assert first.shape == (rows, pitch)
    for r, (n, plan, ids, lp, ref) in enumerate(recs):
        check_row(info[r], first[r], last[r], logp[r], ref, ids, plan.t_total, plan.n_windows, (margin, rows, hole, r))
    # the dict form
    d = eng.align_windows(dev, [r[0] for r in recs], [r[2] for r in recs], window_s=WINDOW / 16000, margin_s=margin * L.HOP / 16000)
    for r, (n, plan, ids, lp, ref) in enumerate(recs):
        assert d[r]["ids"].tolist() == ids.tolist() and d[r]["first"].tolist() == ref["first"].tolist() and d[r]["flags"] == 0
        assert d[r]["last"].tolist() == ref["last"].tolist() and bits(d[r]["score"]) == bits(ref["score"])
        assert (d[r]["n_tokens"], d[r]["t_frames"], d[r]["n_windows"]) == (len(ids), plan.t_total, plan.n_windows)


# ------------------------------------------------------------------ 2. the tie rule ---------------------------------------

def test_tie_rule_on_quantised_log_probs(eng):
    T, n_tok = 150, 60
    rng = np.random.default_rng(20261)
    ids = rng.integers(0, 1024, size=n_tok)
    for i in (1, 5, 6, 30, 59):
        ids[i] = ids[i - 1]                                # adjacent equal tokens: no skip between them
    lp = (np.round(rng.standard_normal((T, 1025)) * 2) / 4 - 3).astype(np.float32)    # multiples of 0.25: equal sums occur
    ref = A.viterbi(lp, ids, ties=True)
    assert ref["flags"] == 0 and float(ref["score"]) * 4 == round(float(ref["score"]) * 4)
    assert len(ref["tie01"]) >= 1 and len(ref["tie12"]) >= 1   # the premise: both ties decide a step of the path itself
    print("ties on the path: stay == s-1 at", len(ref["tie01"]), "frames, s-1 == s-2 at", len(ref["tie12"]))
    n = samples_for(T)
    for margin in (0, 6):
        plan = L.plan(n, MAX_SAMPLES, WINDOW, margin)
        dev = torch.from_numpy(L.cut_logprobs(lp, plan, KW + 1)).cuda().contiguous()
        info, first, last, logp = eng.align_windows_raw(dev, [n], [ids], WINDOW, margin)
        check_row(info[0], first[0], last[0], logp[0], ref, ids, T, plan.n_windows, ("ties", margin))


# ------------------------------------------------------------------ 3. the state layout -----------------------------------

def layout_case(n_tok: int, seed: int):
    """(ids, log-probs [T, 1025], T) with T = L + rep + 40: a planted path of one frame per token (a blank between equal
    neighbours) and 40 more frames among them; adjacent equal tokens every 97 tokens and at both ends"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 1024, size=n_tok)
    for i in sorted(set(range(97, n_tok, 97)) | {1, n_tok - 1}):
        if 1 <= i < n_tok:
            ids[i] = ids[i - 1]
    rep = int(np.sum(ids[1:] == ids[:-1]))
    path = D.path_of(ids.tolist())
    assert len(path) == n_tok + rep
    for pos in sorted(rng.integers(0, len(path) + 1, size=40).tolist(), reverse=True):
        path.insert(pos, BLANK if pos == 0 or pos == len(path) or rng.integers(0, 2) else path[pos - 1])
    T = n_tok + rep + 40
    assert len(path) == T
    lp = (rng.standard_normal((T, 1025), dtype=np.float32) - np.float32(9.0)).astype(np.float32)
    lp[np.arange(T), np.asarray(path)] += np.float32(8.5)
    return ids, lp, T


# around every boundary between two instantiations (2L + 1 = 4096, 8192, 16384: L = 2047 | 2048, 4095 | 4096, 8191 | 8192)
LAYOUT = [1, 2, 31, 32, 383, 384, 1023, 1024, 2046, 2047, 2048, 4094, 4095, 4096, 8190, 8191, 8192]


@pytest.mark.parametrize("n_tok", LAYOUT)
def test_state_layout(eng, n_tok):
    ids, lp, T = layout_case(n_tok, 777 + n_tok)
    ref = A.viterbi(lp, ids)
    assert ref["flags"] == 0
    n = samples_for(T)
    plan = L.plan(n, MAX_SAMPLES, WINDOW, 6)
    assert plan.n_windows >= 2 and plan.t_total == T
    dev = torch.from_numpy(L.cut_logprobs(lp, plan, KW + 1)).cuda().contiguous()
    info, first, last, logp = eng.align_windows_raw(dev, [n], [ids], WINDOW, 6)
    check_row(info[0], first[0], last[0], logp[0], ref, ids, T, plan.n_windows, n_tok)


def test_the_longest_target_on_an_engine_of_default_capacity(big):
    n_tok = A.MAX_TOKENS
    ids, lp, T = layout_case(n_tok, 99)
    ref = A.viterbi(lp, ids)
    assert ref["flags"] == 0 and A.ns_of(n_tok) == 32 and A.threads_of(n_tok) == 1024
    n = samples_for(T)
    plan = L.plan(n, BIG_SAMPLES)
    assert plan.kw == 765 and plan.n_windows >= 2 and plan.t_total == T
    assert big.align_long_plan([n], [n_tok]) == {"n_windows": plan.n_windows, "bytes": A.workspace_bytes([T], [n_tok])}
    dev = torch.from_numpy(L.cut_logprobs(lp, plan, plan.kw + 1)).cuda().contiguous()
    info, first, last, logp = big.align_windows_raw(dev, [n], [ids])
    check_row(info[0], first[0], last[0], logp[0], ref, ids, T, plan.n_windows, n_tok)


def test_a_target_too_long_leaves_the_other_rows_alone(eng):
    cases = [layout_case(31, 5), layout_case(A.MAX_TOKENS + 1, 6), layout_case(32, 7)]
    T = 73                                                  # every row: the first 73 frames of its case
    n = samples_for(T)
    plan = L.plan(n, MAX_SAMPLES, WINDOW, 6)
    dev = torch.from_numpy(np.concatenate([L.cut_logprobs(lp[:T], plan, KW + 1) for _, lp, _ in cases])).cuda().contiguous()
    info, first, last, logp = eng.align_windows_raw(dev, [n] * 3, [c[0] for c in cases], WINDOW, 6)
    assert info["flags"].tolist() == [0, align_ref.TOO_LONG, 0] and first.shape[1] == A.MAX_TOKENS + 1
    for r, (ids, lp, _) in enumerate(cases):
        check_row(info[r], first[r], last[r], logp[r], A.viterbi(lp[:T], ids), ids, T, plan.n_windows, r)


# ------------------------------------------------------------------ 4. equality with qv_align -----------------------------

@pytest.mark.parametrize("n_tok,T,rep", align_ref.PLANTED)
def test_equals_qv_align_on_the_planted_cases(big, n_tok, T, rep):
    """every planted case as a recording of ONE window; (191, 768, 3) has more frames than a window of the largest engine
    holds (766), so that one goes through two windows -- qv_align takes its 768 rows as they are"""
    ids, lp = align_ref.planted_case(n_tok, T, rep)
    n = samples_for(T)
    plan = L.plan(n, BIG_SAMPLES)
    assert plan.t_total == T and plan.n_windows == (2 if T == 768 else 1)
    want = big.align(torch.from_numpy(lp[None]).cuda().contiguous(), [T], [ids])[0]
    dev = torch.from_numpy(L.cut_logprobs(lp, plan, plan.kw + 1)).cuda().contiguous()
    got = big.align_windows(dev, [n], [ids])[0]
    assert want["flags"] == 0 and want["n_tokens"] == n_tok
    assert got.pop("n_windows") == plan.n_windows
    assert want.pop("start") == -1 and want.pop("span") == 0          # (the verse of qv_align_results_ctx: no field of the long record)
    assert got.keys() == want.keys()
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        elif isinstance(want[k], float):
            assert bits(got[k]) == bits(want[k]), k
        else:
            assert got[k] == want[k], k


# ------------------------------------------------------------------ 5. flags and errors -----------------------------------

def test_flags_and_errors(eng, model_eng):
    from offline_tarteel_amd.engine import ALIGN_LONG_INFO_DTYPE

    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tiny = torch.zeros(16, dtype=torch.float32, device="cuda")           # nothing may read it: no launch looks at the inputs
    dev = C.c_void_p(tiny.data_ptr())
    PITCH = 40
    info = np.zeros(5, ALIGN_LONG_INFO_DTYPE)
    first, last, logp = np.full((5, PITCH), 4, np.int32), np.full((5, PITCH), 6, np.int32), np.full((5, PITCH), 3.0, np.float32)

    def reset():
        info["n_tokens"] = -77
        first[:], last[:], logp[:] = 4, 6, 3.0

    def untouched():
        return (info["n_tokens"] == -77).all() and (first == 4).all() and (last == 6).all() and (logp == 3.0).all()

    def windows_call(e, lengths, targets, t_max=KW + 1, window=0, margin=-1, pitch=PITCH, rows=None, tg_null=False):
        ln = np.asarray(lengths, np.int64)
        lens = np.asarray([len(t) for t in targets], np.int32)
        tg = np.concatenate([np.asarray(t, np.uint16) for t in targets] + [np.zeros(1, np.uint16)])
        return e.lib.qv_align_windows(e.h, dev, t_max, p(ln), len(lengths) if rows is None else rows, window, margin,
                                      None if tg_null else p(tg), p(lens), p(info), p(first), p(last), p(logp), pitch, None)

    def long_call(e, lengths, targets, window=0, margin=-1, pitch=PITCH, audio_pitch=None, rows=None):
        ln = np.asarray(lengths, np.int64)
        lens = np.asarray([len(t) for t in targets], np.int32)
        tg = np.concatenate([np.asarray(t, np.uint16) for t in targets] + [np.zeros(1, np.uint16)])
        return e.lib.qv_align_long(e.h, dev, int(max(lengths)) if audio_pitch is None else audio_pitch, p(ln),
                                   len(lengths) if rows is None else rows, window, margin, p(tg), p(lens), p(info), p(first), p(last),
                                   p(logp), pitch, None)

    n = 130003                                                           # 102 frames, 5 windows
    # flags the host decides: the call succeeds, the rows come back flagged, and nothing was launched on the 16 floats
    reset()
    assert windows_call(eng, [n, samples_for(5), samples_for(5)], [[], [7, 7, 7, 9], [1, 2, 3, 4, 5, 6]]) == 0
    assert info["flags"][:3].tolist() == [align_ref.NO_TARGET, align_ref.INFEASIBLE, align_ref.INFEASIBLE]
    assert info["n_tokens"][:3].tolist() == [0, 4, 6] and info["t_frames"][:3].tolist() == [102, 5, 5] and info["n_windows"][:3].tolist() == [5, 1, 1]
    assert (first[:3] == -1).all() and (last[:3] == -1).all() and not logp[:3].any() and not info["score"][:3].any()
    assert (first[3:] == 4).all() and info["n_tokens"][3] == -77
    reset()
    assert long_call(model_eng, [n], [[]]) == 0 and info["flags"][0] == align_ref.NO_TARGET and (first[0] == -1).all()
    torch.cuda.synchronize()
    # errors: nothing is written
    reset()
    ok = [5, 6, 7]
    assert long_call(eng, [n], [ok]) == ERR_NO_MODEL and b"model" in eng.lib.qv_last_error(eng.h)
    m = model_eng
    top = L.HOP * L.MAX_FRAMES
    assert long_call(m, [n] * 5, [ok] * 5) == ERR_CAPACITY                               # rows > max_batch
    assert long_call(m, [top], [ok]) == ERR_CAPACITY                                     # T above QV_LONG_MAX_FRAMES
    assert long_call(m, [n], [ok], window=WINDOW, margin=19) == ERR_ARG                  # H < 1
    assert long_call(m, [n], [ok], window=WINDOW - 1) == ERR_ARG                         # not a multiple of 1280
    assert long_call(m, [n], [ok], window=WINDOW + L.HOP) == ERR_ARG                     # above max_samples
    assert long_call(m, [n], [ok], pitch=2) == ERR_ARG                                   # pitch below the largest L
    assert long_call(m, [n], [ok], audio_pitch=n - 1) == ERR_ARG                         # a recording longer than its row
    assert long_call(m, [n], [ok], rows=0) == ERR_ARG
    assert long_call(m, [n], [[5, 1024, 7]]) == ERR_ARG                                  # an id outside 0..1023
    assert long_call(m, [399], [ok]) == ERR_CAPACITY                                     # below the forward's minimum
    ln, lens, tg = np.array([n], np.int64), np.array([3], np.int32), np.array(ok, np.uint16)
    full = [m.h, dev, n, p(ln), 1, 0, -1, p(tg), p(lens), p(info), p(first), p(last), p(logp), PITCH, None]
    for k in (1, 3, 8, 9, 10, 11, 12):                                                   # audio, lengths, lens and every output
        assert m.lib.qv_align_long(*[None if i == k else a for i, a in enumerate(full)]) == ERR_ARG, k
    assert m.lib.qv_align_long(*[None if i == 7 else a for i, a in enumerate(full)]) == ERR_ARG   # targets with tokens to read
    big_rows = [L.HOP * L.MAX_FRAMES - 1] * 2
    for e in (eng, m):
        assert windows_call(e, [n] * 5, [ok] * 5) == ERR_CAPACITY
        assert windows_call(e, [top], [ok]) == ERR_CAPACITY
        assert windows_call(e, [n], [ok], window=WINDOW, margin=19) == ERR_ARG
        assert windows_call(e, [n], [ok], window=1000) == ERR_ARG
        assert windows_call(e, [n], [ok], pitch=2) == ERR_ARG
        assert windows_call(e, [n], [ok], t_max=KW) == ERR_ARG                           # the tensor cannot hold a window's frames
        assert windows_call(e, [n], [ok], rows=0) == ERR_ARG
        assert windows_call(e, [n], [[1024]]) == ERR_ARG
        assert windows_call(e, [n], [ok], tg_null=True) == ERR_ARG
        # two recordings of the most frames against the longest target: above QV_ALIGN_LONG_MAX_BYTES
        assert windows_call(e, big_rows, [[5] * A.MAX_TOKENS] * 2, pitch=A.MAX_TOKENS) == ERR_CAPACITY
        assert b"QV_ALIGN_LONG_MAX_BYTES" in e.lib.qv_last_error(e.h)
    assert untouched()
    with pytest.raises(Exception):
        eng.align_long_plan(big_rows, [A.MAX_TOKENS] * 2)


# ------------------------------------------------------------------ 6. the audio API --------------------------------------

def window_logprobs(e, recordings, plans, t_max):
    """every window of every recording through Engine.forward, three at a time in reversed order (a grouping the long path's
    rounds never use): float32 [windows, t_max, 1025] in recording-then-window order, NaN behind a window's frames"""
    jobs = [(r, w) for r, p in enumerate(plans) for w in range(p.n_windows)]
    at = {j: k for k, j in enumerate(jobs)}
    out = np.full((len(jobs), t_max, 1025), np.nan, np.float32)
    rev = jobs[::-1]
    for s in range(0, len(rev), 3):
        part = rev[s: s + 3]
        buf = np.zeros((len(part), WINDOW), np.float32)
        lens = []
        for k, (r, w) in enumerate(part):
            x = L.cut_audio(recordings[r], plans[r])[w]
            buf[k, : len(x)] = x
            lens.append(plans[r].fwd_length(w))
        lp, T = e.forward(torch.from_numpy(buf).cuda(), lens)
        lp = lp.cpu().numpy()
        for k, (r, w) in enumerate(part):
            assert T[k] == L.frames(plans[r].length(w))
            out[at[(r, w)], : T[k]] = lp[k, : T[k]]
    return out


@pytest.mark.parametrize("lengths,margin", [((48000, 48001, 49279, 130003), -1), ((211007,), -1), ((2 * WINDOW + 100, 130003), 0)])
def test_audio_api_equals_the_windows_api_on_the_engines_own_windows(model_eng, lengths, margin):
    e = model_eng
    n_top = max(lengths)
    host = synth_audio(len(lengths), n_top, seed=20260700 + margin)
    for b, n in enumerate(lengths):
        host[b, n:] = 0.0
    plans = [L.plan(n, MAX_SAMPLES, 0, margin) for n in lengths]
    assert all(p.kw == KW and p.n_windows >= 2 for p in plans)
    audio = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    before = e.transcribe_long_raw(audio, list(lengths), 0, margin)
    # targets: the recordings' own greedy tokens, so a path exists
    targets = [before[1][r, : int(before[0][r]["n_tokens"])].astype(np.int64) for r in range(len(lengths))]
    assert any(len(t) for t in targets) and all((t >= 0).all() and (t < 1024).all() for t in targets)
    got = e.align_long_raw(audio, list(lengths), targets, 0, margin)
    wl = window_logprobs(e, host, plans, KW + 1)
    want = e.align_windows_raw(torch.from_numpy(wl).cuda().contiguous(), list(lengths), targets, 0, margin)
    for a, b, name in zip(got, want, ("info", "first", "last", "logp")):
        assert a.tobytes() == b.tobytes(), name
    for r, t in enumerate(targets):
        assert int(got[0][r]["flags"]) == (0 if len(t) else align_ref.NO_TARGET) and int(got[0][r]["n_windows"]) == plans[r].n_windows
        if len(t):      # ... and both equal the restatement on the stitched rows
            off = sum(p.n_windows for p in plans[:r])
            ref = A.viterbi(A.stitched(wl[off: off + plans[r].n_windows], plans[r]), t)
            check_row(got[0][r], got[1][r], got[2][r], got[3][r], ref, t, plans[r].t_total, plans[r].n_windows, (lengths, r))
    after = e.transcribe_long_raw(audio, list(lengths), 0, margin)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 7. end to end -----------------------------------------

class ServedEngine:
    """the engine, with transcribe_long and align_long answering from prepared GLOBAL log-probs cut into window tensors (NaN
    wherever the long path must not look) through the real qv_transcribe_windows / qv_align_windows"""

    def __init__(self, eng, served: dict):
        self._eng, self._served, self.calls = eng, served, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def _cut(self, audio, lengths):
        assert audio.is_cuda and tuple(audio.shape) == (1, int(lengths[0]))
        n = int(lengths[0])
        plan = L.plan(n, self._eng.max_samples)
        return n, plan, torch.from_numpy(L.cut_logprobs(self._served[n], plan, plan.kw + 1)).cuda().contiguous()

    def transcribe_batch(self, audio, lengths, confidence=False):
        raise AssertionError("a recording above the engine's capacity must take the long path")

    def transcribe_long(self, audio, lengths, window_s=None, margin_s=None):
        n, plan, cut = self._cut(audio, lengths)
        self.calls.append(("transcribe", plan.n_windows))
        return self._eng.transcribe_windows(cut, [n])

    def align_long(self, audio, lengths, targets, window_s=None, margin_s=None):
        n, plan, cut = self._cut(audio, lengths)
        self.calls.append(("align", plan.n_windows))
        return self._eng.align_windows(cut, [n], targets)


def test_three_ayat_end_to_end_with_timings(eng, oracle, monkeypatch):
    from offline_tarteel_amd import plugin
    from offline_tarteel_amd.streaming import StreamingPipeline
    from offline_tarteel_amd.words import FRAME_SECONDS, verses_from_alignment

    verses = [(2, 2), (2, 3), (2, 4)]
    start = eng.tables.verse_index(2, 2)
    ids, ends = eng.tables.range_token_ids(start, 3)
    assert ids.tolist() == [i for s, a in verses for i in oracle.token_ids(oracle.verse_index(s, a), 1).tolist()]
    unit = D.path_of(ids.tolist())
    rep = -(-170 // len(unit))                                   # every token several frames long: about 170 frames in all
    path = [BLANK] * 3 + [i for i in unit for _ in range(rep)] + [BLANK] * 4
    T = len(path)
    n = samples_for(T)
    assert T >= 4 * (KW + 1) and n > 4 * MAX_SAMPLES             # several windows
    lp = D.frames_of(path, 7700)
    # where each ayah was planted: the first frame of its first token
    tok_at = [k for k, (a, b) in enumerate(zip([BLANK] + path[:-1], path)) if b != BLANK and a != b]
    assert len(tok_at) == len(ids)
    planted = [tok_at[0]] + [tok_at[int(e)] for e in ends[:-1]]
    plan = L.plan(n, MAX_SAMPLES)
    cut = torch.from_numpy(L.cut_logprobs(lp, plan, plan.kw + 1)).cuda().contiguous()
    row = eng.align_windows(cut, [n], [ids])[0]
    assert row["flags"] == 0 and row["n_windows"] == plan.n_windows >= 6 and row["t_frames"] == T
    out = verses_from_alignment(eng.tables, range(start, start + 3), ends, row)
    assert [(v["surah"], v["ayah"]) for v in out] == verses
    for v, at in zip(out, planted):
        assert abs(v["start"] / FRAME_SECONDS - at) <= 1, (v["ayah"], v["start"], at)      # within one frame of where it was planted
        assert v["end"] > v["start"] and v["words"] and v["start"] == v["words"][0]["start"] and v["end"] == v["words"][-1]["end"]
    assert all(a["end"] <= b["start"] for a, b in zip(out, out[1:]))
    # predict_long on a stub engine: the emissions as they are today, and with timings the same emissions plus three keys
    served = ServedEngine(eng, {n: lp})
    monkeypatch.setattr(plugin, "_engine", served)
    monkeypatch.setattr(plugin, "_LONG_TIMINGS", False)
    recording = np.zeros(n, np.float32)
    today = StreamingPipeline(served).run_on_full_transcript(recording)
    assert [(g["surah"], g["ayah"]) for g in today] == verses
    assert plugin.predict_long(recording) == today == plugin.predict_long(recording, timings=False)
    assert all(kind == "transcribe" for kind, _ in served.calls)
    timed = plugin.predict_long(recording, timings=True)
    assert served.calls[-1] == ("align", plan.n_windows)
    assert [{k: g[k] for k in ("surah", "ayah", "score")} for g in timed] == today
    assert all(set(g) == {"surah", "ayah", "score", "start", "end", "logp"} for g in timed)
    for g, v in zip(timed, out):
        assert (g["start"], g["end"], g["logp"]) == (v["start"], v["end"], v["logp"])
    monkeypatch.setattr(plugin, "_LONG_TIMINGS", True)           # QVERSE_LONG_TIMINGS=1
    assert plugin.predict_long(recording) == timed
