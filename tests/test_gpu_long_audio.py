"""Recordings of any length (csrc/qv_long.hip: k_long_gather, k_long_frames, k_long_collapse; include/qverse.h
qv_transcribe_long / qv_transcribe_windows) on the MI355X.

What is pinned, bit for bit: the long path equals "the existing engine on every window separately, stitched by the
documented rule (tests/long_ref.py, held to csrc/qv_long_plan.h by tests/test_long_plan_host.py), collapsed by
qv_transcribe's documented rule (tests/transcribe_ref.py)".  How close a windowed transcript comes to ONE forward over the
whole recording is not a subject of these tests (unmeasured).

The engines are small: max_samples = 48,000 (windows of 37 frames = 47,360 samples, 38 frames each) and max_batch = 4."""

import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as D
import long_ref as L
import transcribe_ref as R
from synth import BLANK, VOCAB, hash_noise, synth_audio

pytestmark = pytest.mark.gpu

MAX_SAMPLES = 48000
KW = 37
WINDOW = KW * L.HOP
ERR_ARG, ERR_CAPACITY, ERR_NO_MODEL = 1, 4, 5


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=4, max_samples=MAX_SAMPLES)
    assert e.frames_for(WINDOW) == KW + 1 and e.long_plan_raw(WINDOW + 1)["kw"] == KW
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=True, seed=11, max_batch=4, max_samples=MAX_SAMPLES)
    yield e
    e.close()


def samples_for(T: int) -> int:
    return (T - 1) * L.HOP + 640


def rows_of(info, ids, logp, first, last):
    """per recording the fields in comparable form (floats as their bytes)"""
    out = []
    for b in range(len(info)):
        n = int(info[b]["n_tokens"])
        out.append({"ids": ids[b, :n].tolist(), "first": first[b, :n].tolist(), "last": last[b, :n].tolist(),
                    "logp": logp[b, :n].tobytes(), "n_tokens": n, "t_frames": int(info[b]["t_frames"]),
                    "n_blank_frames": int(info[b]["n_blank_frames"]), "flags": int(info[b]["flags"]),
                    "n_windows": int(info[b]["n_windows"]), "reserved": int(info[b]["reserved"]),
                    "min_token_logprob": info[b]["min_token_logprob"].tobytes(), "reserved_f": float(info[b]["reserved_f"]),
                    "avg_logprob": info[b]["avg_logprob"].tobytes(), "frame_avg_logprob": info[b]["frame_avg_logprob"].tobytes(),
                    "tail": (ids[b, n:].tolist(), first[b, n:].tolist(), last[b, n:].tolist(), logp[b, n:].tobytes())})
    return out


def check(got: dict, ref: dict, n_windows: int, tag):
    want = {"ids": ref["ids"], "first": ref["first"], "last": ref["last"], "logp": R.bits32(ref["logp"]),
            "n_tokens": ref["n_tokens"], "t_frames": ref["t_frames"], "n_blank_frames": ref["n_blank_frames"],
            "flags": ref["flags"], "n_windows": n_windows, "reserved": 0,
            "min_token_logprob": R.bits32(ref["min_token_logprob"]), "reserved_f": 0.0,
            "avg_logprob": R.bits64(ref["avg_logprob"]), "frame_avg_logprob": R.bits64(ref["frame_avg_logprob"])}
    for k, v in want.items():
        assert got[k] == v, (tag, k, got[k], v)
    pad = len(got["tail"][0])
    assert got["tail"] == ([-1] * pad, [-1] * pad, [-1] * pad, np.zeros(pad, np.float32).tobytes()), tag


# ------------------------------------------------------------------ 1. the windows API on crafted log-probs ----------------

def crafted(T: int, plan: L.Plan, seed: int):
    """a global frame path of T frames with, on the first five seams of the plan (a seam = the first frame a window other
    than the first owns): a token run across it, a blank run across it, the same id on both sides with nothing between (one
    token), the same id on both sides of an owned blank (two tokens), and a run whose maximum lies in the later window.
    Returns (log-probs float32 [T, 1025], {feature: seam})."""
    fill = [100 + k % 90 if k % 5 else BLANK for k in range(T)]          # one-frame tokens, a blank every fifth frame
    path = [fill[t] if t % 3 else fill[min(t + 1, T - 1)] for t in range(T)]   # ... some of them two frames long
    seams = [plan.lo(w) for w in range(1, plan.n_windows)]
    assert len(seams) >= 5 and all(b - a >= 1 for a, b in zip(seams, seams[1:]))
    far = [s for s in seams if 3 <= s <= T - 4]
    pick = [far[0]]
    for s in far[1:]:
        if s - pick[-1] >= 7 and len(pick) < 5:        # features do not touch one another
            pick.append(s)
    assert len(pick) == 5, (pick, seams)
    a, b, c, d, e = pick
    path[a - 2: a + 2] = [300] * 4                                       # token run across the seam
    path[b - 2: b + 2] = [BLANK] * 4                                     # blank run across the seam
    path[c - 2: c + 2] = [301, 302, 302, 303]                            # 302 | 302: one token
    path[d - 2: d + 2] = [304, 305, BLANK, 305]                          # 305 | blank (owned by the later window) 305: two tokens
    path[e - 2: e + 3] = [306] * 5                                       # the maximum of this run: frame e + 1
    lp = D.frames_of(path, seed)
    lg = hash_noise((1, VOCAB), seed + 5000)
    lg[0, 306] += np.float32(20.0)                                       # a frame surer of its token than every other
    lp[e + 1] = D.log_softmax32(lg)[0]
    return np.ascontiguousarray(lp, np.float32), dict(zip("abcde", pick))


def premises(ref: dict, at: dict):
    tok = {(i, f, l) for i, f, l in zip(ref["ids"], ref["first"], ref["last"])}
    a, b, c, d, e = (at[k] for k in "abcde")
    assert (300, a - 2, a + 1) in tok                                              # one token across the seam
    assert (ref["fid"][b - 2: b + 2] == BLANK).all()
    assert (302, c - 1, c) in tok and sum(i == 302 for i in ref["ids"]) == 1
    assert (305, d - 1, d - 1) in tok and (305, d + 1, d + 1) in tok and ref["fid"][d] == BLANK
    k = ref["ids"].index(306)
    assert (ref["first"][k], ref["last"][k]) == (e - 2, e + 2)
    assert int(np.argmax(ref["m"][e - 2: e + 3])) == 3 and R.bits32(ref["logp"][k]) == R.bits32(ref["m"][e + 1])


@pytest.fixture(scope="module")
def crafted_cases():
    """{margin: [(n, plan, lp, ref)]}: three ragged recordings per margin -- 200 frames, one window, 193 frames"""
    out = {}
    for margin in (6, 0, 18):
        recs = []
        for k, T in enumerate((200, 38, 193)):
            n = WINDOW if T == 38 else samples_for(T)
            plan = L.plan(n, MAX_SAMPLES, WINDOW, margin)
            assert plan.t_total == T and plan.h == KW - 2 * margin
            if T == 38:
                assert plan.n_windows == 1
                lp = D.frames_of([7, 7, BLANK, 7] + [BLANK] * 30 + [9, 9, 8, 8], 4100 + margin)
            else:
                lp, at = crafted(T, plan, 4000 + 10 * margin + k)
            ref = R.transcribe_ref(lp, T)
            if T != 38:
                premises(ref, at)
            recs.append((n, plan, lp, ref))
        out[margin] = recs
    assert out[6][0][1].n_windows == 8 and out[0][0][1].n_windows == 6 and out[18][0][1].n_windows == 164   # > 4: two rounds and more
    return out


@pytest.mark.parametrize("margin", [6, 0, 18])
@pytest.mark.parametrize("rows", [1, 3])
def test_windows_api_on_crafted_log_probs(eng, crafted_cases, margin, rows):
    recs = crafted_cases[margin][:rows]
    t_max = KW + 1 + (3 if rows == 3 else 0)           # the tensor may be longer than a window
    cut = np.concatenate([L.cut_logprobs(lp, plan, t_max) for _, plan, lp, _ in recs])
    assert np.isnan(cut).any() and cut.shape[0] == sum(plan.n_windows for _, plan, _, _ in recs)
    dev = torch.from_numpy(cut).cuda().contiguous()
    pitch = 200 + (5 if rows == 3 else 0)
    got = rows_of(*eng.transcribe_windows_raw(dev, [n for n, _, _, _ in recs], WINDOW, margin, pitch=pitch))
    for r, (n, plan, _, ref) in enumerate(recs):
        assert len(got[r]["tail"][0]) == pitch - ref["n_tokens"]
        check(got[r], ref, plan.n_windows, (margin, rows, r))
    # the dict form: the same tokens, the text of the ids, the window count
    d = eng.transcribe_windows(dev, [n for n, _, _, _ in recs], window_s=WINDOW / 16000, margin_s=margin * L.HOP / 16000)
    for r, (n, plan, _, ref) in enumerate(recs):
        assert [k["id"] for k in d[r]["tokens"]] == ref["ids"] and d[r]["n_windows"] == plan.n_windows
        assert [(k["first"], k["last"]) for k in d[r]["tokens"]] == list(zip(ref["first"], ref["last"]))
        assert d[r]["text"] == eng.transcript_of(ref["ids"]) and R.bits64(d[r]["avg_logprob"]) == R.bits64(ref["avg_logprob"])


@pytest.mark.parametrize("T", [1024, 1025, 2500])
def test_collapse_slabs_of_several_chunks(eng, T):
    """k_long_collapse gives each of its sixteen waves a slab of ceil(ceil(T / 64) / 16) chunks: one chunk up to T = 1024, two
    from 1025 on, three at T = 2500 (slabs of 192 frames, the last one short).  Runs that cross slab edges, a run that covers
    a whole slab (a slab without a run start only carries a maximum through), maxima before, inside and behind that slab."""
    slab = -(-(-(-T // 64)) // 16) * 64
    assert slab == {1024: 64, 1025: 128, 2500: 192}[T]
    path = [100 + k % 90 if k % 7 else BLANK for k in range(T)]
    s = slab
    path[s - 5: s + 9] = [400] * 14                       # across the first slab edge
    path[2 * s - 3: 2 * s + 3] = [BLANK] * 6              # a blank run across the second
    path[3 * s - 10: 5 * s + 10] = [401] * (2 * s + 20)   # covers the fourth and fifth slab whole
    path[5 * s + 10] = 402
    path[6 * s - 1: 6 * s + 1] = [403, 403]               # two frames, one on each side
    path[7 * s - 1: 7 * s + 1] = [404, 405]               # a token ends where the slab does
    cases = []
    for k, peak in enumerate((3 * s - 8, 4 * s + 17, 5 * s + 9)):    # the long run's maximum: before, inside, behind the covered slabs
        lp = D.frames_of(path, 8800 + T + k)
        lg = hash_noise((1, VOCAB), 8900 + k)
        lg[0, 401] += np.float32(20.0)
        lp[peak] = D.log_softmax32(lg)[0]
        ref = R.transcribe_ref(lp, T)
        i = ref["ids"].index(401)
        assert (ref["first"][i], ref["last"][i]) == (3 * s - 10, 5 * s + 9) and R.bits32(ref["logp"][i]) == R.bits32(lp[peak, 401])
        assert (400, s - 5, s + 8) in set(zip(ref["ids"], ref["first"], ref["last"]))
        cases.append((lp, ref))
    n = samples_for(T)
    for margin in (0, 9):
        plan = L.plan(n, MAX_SAMPLES, WINDOW, margin)
        cut = np.concatenate([L.cut_logprobs(lp, plan, KW + 1) for lp, _ in cases])
        got = rows_of(*eng.transcribe_windows_raw(torch.from_numpy(cut).cuda().contiguous(), [n] * 3, WINDOW, margin))
        for r, (_, ref) in enumerate(cases):
            check(got[r], ref, plan.n_windows, (T, margin, r))


def test_the_longest_recording_the_call_accepts(eng):
    """T = QV_LONG_MAX_FRAMES = 262,144 frames (5.8 hours), 7,085 windows, 256 chunks per wave of the collapse: indices
    and offsets at their largest.  The log-probs are made on the device (runs of three frames, blanks among them); the
    expectation is transcribe_ref's own pieces applied to the per-frame maxima, which torch takes from the global matrix."""
    T = L.MAX_FRAMES
    n = L.HOP * T - 1
    plan = L.plan(n, MAX_SAMPLES, WINDOW, 0)
    assert plan.t_total == T and plan.n_windows == 7085
    g = torch.Generator(device="cuda").manual_seed(5)
    path = torch.randint(0, VOCAB, ((T + 2) // 3,), generator=g, device="cuda").repeat_interleave(3)[:T]
    lg = torch.randn((T, VOCAB), generator=g, device="cuda")
    lg[torch.arange(T, device="cuda"), path] += 12.0
    lp = torch.log_softmax(lg, -1)
    del lg
    idx = torch.arange(plan.n_windows, device="cuda")[:, None] * plan.h + torch.arange(KW + 1, device="cuda")[None, :]
    cut = lp[idx.clamp_(max=T - 1)].contiguous()          # (frames past the end of the last window: never read)
    m, fid = lp.max(dim=1)
    assert torch.equal(fid, path)                         # no ties: the argmax is the path whichever maximum torch takes
    fid, m = fid.cpu().numpy(), m.cpu().numpy()
    del lp
    info, ids, logp, first, last = eng.transcribe_windows_raw(cut, [n], WINDOW, 0)
    runs = [(i, a, e) for i, a, e in R.runs_of(fid) if i != BLANK]
    tok = np.asarray([m[a: e + 1][int(np.argmax(m[a: e + 1]))] for _, a, e in runs], np.float32)
    k = len(runs)
    assert 80000 < k == int(info[0]["n_tokens"]) and int(info[0]["t_frames"]) == T and int(info[0]["n_windows"]) == 7085
    assert int(info[0]["n_blank_frames"]) == int((fid == BLANK).sum()) > 0 and int(info[0]["flags"]) == 0
    assert np.array_equal(ids[0, :k], [i for i, _, _ in runs]) and (ids[0, k:] == -1).all()
    assert np.array_equal(first[0, :k], [a for _, a, _ in runs]) and np.array_equal(last[0, :k], [e for _, _, e in runs])
    assert logp[0, :k].tobytes() == tok.tobytes() and not logp[0, k:].any()
    assert info[0]["min_token_logprob"].tobytes() == R.bits32(tok[int(np.argmin(tok))])
    assert info[0]["avg_logprob"].tobytes() == R.bits64(R.lane_sum(tok) / np.float64(k))
    assert info[0]["frame_avg_logprob"].tobytes() == R.bits64(R.lane_sum(m) / np.float64(T))


def test_windows_api_null_optional_arrays(eng, crafted_cases):
    from offline_tarteel_amd.engine import LONG_INFO_DTYPE

    n, plan, lp, ref = crafted_cases[6][0]
    dev = torch.from_numpy(L.cut_logprobs(lp, plan, KW + 1)).cuda().contiguous()
    info, ids = np.zeros(1, LONG_INFO_DTYPE), np.full((1, 200), 7, np.int32)
    ln = np.array([n], np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = eng.lib.qv_transcribe_windows(eng.h, C.c_void_p(dev.data_ptr()), KW + 1, p(ln), 1, WINDOW, 6, p(info), p(ids), None, None, None,
                                       200, None)
    assert rc == 0 and ids[0, : ref["n_tokens"]].tolist() == ref["ids"] and (ids[0, ref["n_tokens"]:] == -1).all()
    assert info[0]["avg_logprob"].tobytes() == R.bits64(ref["avg_logprob"])


# ------------------------------------------------------------------ 2. the audio API against the existing engine ----------

def stitched_reference(e, recordings, plans, group: int = 3):
    """every window of every recording through the existing Engine.forward, `group` windows at a time in REVERSED order (a
    grouping the long path's rounds never use), the owned frames stitched in numpy, transcribe_ref on the result"""
    jobs = [(r, w) for r, p in enumerate(plans) for w in range(p.n_windows)][::-1]
    lps = {}
    for s in range(0, len(jobs), group):
        part = jobs[s: s + group]
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
            lps[(r, w)] = lp[k, : T[k]].copy()
    out = []
    for r, p in enumerate(plans):
        out.append(R.transcribe_ref(L.stitch([lps[(r, w)] for w in range(p.n_windows)], p), p.t_total))
    return out


@pytest.mark.parametrize("lengths,margin", [((48000, 48001, 49279, 130003), -1), ((211007,), -1), ((2 * WINDOW + 100, 130003), 0)])
def test_audio_api_equals_the_existing_engine_window_by_window(model_eng, lengths, margin):
    e = model_eng
    n_top = max(lengths)
    host = synth_audio(len(lengths), n_top, seed=20260700 + margin)
    for b, n in enumerate(lengths):
        host[b, n:] = 0.0
    plans = [L.plan(n, MAX_SAMPLES, 0, margin) for n in lengths]
    assert all(p.kw == KW and p.m == (9 if margin < 0 else margin) and p.n_windows >= 2 for p in plans)
    if margin == 0:
        assert plans[0].length(2) == 100 and plans[0].fwd_length(2) == 400        # the last window below the forward's minimum
    refs = stitched_reference(e, host, plans)
    audio = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    got = rows_of(*e.transcribe_long_raw(audio, list(lengths), 0, margin))
    for r, (p, ref) in enumerate(zip(plans, refs)):
        assert ref["t_frames"] == e.frames_for(lengths[r])
        check(got[r], ref, p.n_windows, (lengths, r))
    # a source the 16-byte loads cannot be used on: the same bits
    odd = torch.zeros(len(lengths) * (n_top + 1) + 1, dtype=torch.float32, device="cuda")
    view = odd[1:].view(len(lengths), n_top + 1)
    view[:, :n_top] = audio
    from offline_tarteel_amd.engine import LONG_INFO_DTYPE

    t_top = L.frames(n_top)
    info = np.zeros(len(lengths), LONG_INFO_DTYPE)
    ids, logp = np.zeros((len(lengths), t_top), np.int32), np.zeros((len(lengths), t_top), np.float32)
    first, last = np.zeros((len(lengths), t_top), np.int32), np.zeros((len(lengths), t_top), np.int32)
    ln = np.asarray(lengths, np.int64)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = e.lib.qv_transcribe_long(e.h, C.c_void_p(view.data_ptr()), n_top + 1, p_(ln), len(lengths), 0, margin, p_(info), p_(ids), p_(logp),
                                  p_(first), p_(last), t_top, None)
    assert rc == 0 and view.data_ptr() % 16 != 0
    assert rows_of(info, ids, logp, first, last) == got


# ------------------------------------------------------------------ 3. one window: today's call ---------------------------

def test_one_window_equals_transcribe_batch(model_eng):
    e = model_eng
    lengths = [16000, 27200, WINDOW]
    host = synth_audio(3, WINDOW)
    for b, n in enumerate(lengths):
        host[b, n:] = 0.0
    audio = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    want = e.transcribe_batch(audio, lengths, confidence=True)
    got = e.transcribe_long(audio, lengths)
    assert [g.pop("n_windows") for g in got] == [1, 1, 1]
    for b in range(3):
        assert got[b].keys() == want[b].keys()
        for k in want[b]:
            if isinstance(want[b][k], float):
                assert R.bits64(got[b][k]) == R.bits64(want[b][k]), (b, k)
            elif k == "tokens":
                assert [(t["id"], t["first"], t["last"], R.bits32(t["logp"])) for t in got[b][k]] == [
                    (t["id"], t["first"], t["last"], R.bits32(t["logp"])) for t in want[b][k]], b
            else:
                assert got[b][k] == want[b][k], (b, k)
    assert any(w["n_tokens"] for w in want)


# ------------------------------------------------------------------ 4. errors ---------------------------------------------

def test_error_paths(eng, model_eng):
    from offline_tarteel_amd.engine import LONG_INFO_DTYPE

    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tiny = torch.zeros(16, dtype=torch.float32, device="cuda")
    info = np.zeros(5, LONG_INFO_DTYPE)
    info["n_tokens"] = -77
    ids, logp = np.full((5, 300), 5, np.int32), np.full((5, 300), 3.0, np.float32)
    first, last = np.full((5, 300), 4, np.int32), np.full((5, 300), 6, np.int32)
    dev = C.c_void_p(tiny.data_ptr())

    def long_call(e, lengths, window=0, margin=-1, pitch=300, audio_pitch=None, rows=None):
        ln = np.asarray(lengths, np.int64)
        return e.lib.qv_transcribe_long(e.h, dev, int(max(lengths)) if audio_pitch is None else audio_pitch, p(ln),
                                        len(lengths) if rows is None else rows, window, margin, p(info), p(ids), p(logp), p(first),
                                        p(last), pitch, None)

    def windows_call(e, lengths, t_max=KW + 1, window=0, margin=-1, pitch=300):
        ln = np.asarray(lengths, np.int64)
        return e.lib.qv_transcribe_windows(e.h, dev, t_max, p(ln), len(lengths), window, margin, p(info), p(ids), p(logp), p(first),
                                           p(last), pitch, None)

    n = 130003                                                                     # 102 frames
    assert long_call(eng, [n]) == ERR_NO_MODEL and b"model" in eng.lib.qv_last_error(eng.h)
    m = model_eng
    assert long_call(m, [n] * 5) == ERR_CAPACITY                                   # rows > max_batch
    top = L.HOP * L.MAX_FRAMES
    assert long_call(m, [top]) == ERR_CAPACITY                                     # T above QV_LONG_MAX_FRAMES: refused before any launch
    assert long_call(m, [n], window=WINDOW, margin=19) == ERR_ARG                  # H < 1
    assert long_call(m, [n], window=WINDOW - 1) == ERR_ARG                         # not a multiple of 1280
    assert long_call(m, [n], window=WINDOW + L.HOP) == ERR_ARG                     # above max_samples
    assert long_call(m, [n], pitch=101) == ERR_ARG                                 # pitch < T
    assert long_call(m, [n], audio_pitch=n - 1) == ERR_ARG                         # a recording longer than its row
    assert long_call(m, [n], rows=0) == ERR_ARG
    assert m.lib.qv_transcribe_long(m.h, None, n, p(np.array([n], np.int64)), 1, 0, -1, p(info), p(ids), None, None, None, 300, None) == ERR_ARG
    assert m.lib.qv_transcribe_long(m.h, dev, n, p(np.array([n], np.int64)), 1, 0, -1, None, p(ids), None, None, None, 300, None) == ERR_ARG
    for e in (eng, m):
        assert windows_call(e, [n] * 5) == ERR_CAPACITY
        assert windows_call(e, [top]) == ERR_CAPACITY
        assert windows_call(e, [n], window=WINDOW, margin=19) == ERR_ARG
        assert windows_call(e, [n], window=1000) == ERR_ARG
        assert windows_call(e, [n], pitch=101) == ERR_ARG
        assert windows_call(e, [n], t_max=KW) == ERR_ARG                           # the tensor cannot hold a window's frames
    # nothing ran: the output arrays are as they were
    assert (info["n_tokens"] == -77).all() and (ids == 5).all() and (logp == 3.0).all() and (first == 4).all() and (last == 6).all()
    with pytest.raises(Exception):
        eng.long_plan(n, margin_s=19 * L.HOP / 16000)
    assert eng.long_plan(n) == {"n_windows": 5, "t_frames": 102, "kw": KW, "margin_frames": 9, "hop_frames": 19, "window_samples": WINDOW}


# ------------------------------------------------------------------ 5. end to end -----------------------------------------

class ServedLongEngine:
    """the engine, with transcribe_long answering from prepared GLOBAL log-probs cut into window tensors (NaN wherever the
    long path must not look) through the real qv_transcribe_windows; everything else is the engine's"""

    def __init__(self, eng, served: dict):
        self._eng, self._served, self.calls = eng, served, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def transcribe_batch(self, audio, lengths, confidence=False):
        raise AssertionError("a recording above the engine's capacity must take the long path")

    def transcribe_long(self, audio, lengths, window_s=None, margin_s=None):
        assert audio.is_cuda and tuple(audio.shape) == (1, int(lengths[0])) and window_s is None and margin_s is None
        n = int(lengths[0])
        plan = L.plan(n, self._eng.max_samples)
        self.calls.append(plan.n_windows)
        cut = L.cut_logprobs(self._served[n], plan, plan.kw + 1)
        return self._eng.transcribe_windows(torch.from_numpy(cut).cuda().contiguous(), [n])


def test_three_ayat_end_to_end(eng, model_eng, oracle):
    from offline_tarteel_amd.engine import QvError
    from offline_tarteel_amd.streaming import StreamingPipeline

    verses = [(2, 2), (2, 3), (2, 4)]      # (the reference's peeling emits exactly these for their text: the oracle agrees)
    ids = [i for s, a in verses for i in oracle.token_ids(oracle.verse_index(s, a), 1).tolist()]
    unit = D.path_of(ids)
    rep = -(-170 // len(unit))                                   # every token several frames long: about 170 frames in all
    path = [BLANK] * 3 + [i for i in unit for _ in range(rep)] + [BLANK] * 4
    T = len(path)
    n = samples_for(T)
    assert T >= 4 * (KW + 1) and n > 4 * MAX_SAMPLES             # longer than one 3-s window several times over
    lp = D.frames_of(path, 7700)
    ref = R.transcribe_ref(lp, T)
    assert ref["ids"] == ids
    served = ServedLongEngine(eng, {n: lp})
    recording = np.zeros(n, np.float32)
    got = StreamingPipeline(served).run_on_full_transcript(recording)
    assert [(g["surah"], g["ayah"]) for g in got] == verses      # exactly those ayat
    assert got == StreamingPipeline(eng).run_on_full_transcript("x.wav", lambda p: eng.transcript_of(ids))
    assert served.calls == [L.plan(n, MAX_SAMPLES).n_windows] and served.calls[0] >= 6
    # on an engine whose capacity the recording exceeds, today's path raises and the new one answers
    audio = torch.from_numpy(synth_audio(1, n)).cuda()
    with pytest.raises(QvError):
        model_eng.transcribe_batch(audio, [n], confidence=True)
    with pytest.raises(QvError):
        model_eng.transcribe_batch(audio, [n])
    out = model_eng.transcribe_long(audio, [n])[0]
    assert out["t_frames"] == T and out["n_windows"] == served.calls[0] and out["n_tokens"] == len(out["tokens"])
    assert isinstance(StreamingPipeline(model_eng).run_on_full_transcript(synth_audio(1, n)[0]), list)
