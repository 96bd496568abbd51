"""Ranked alternatives selected on the device (csrc/qv_nbest.hip: qv_nbest_select, qv_nbest_results_ctx) against the
restatement (tests/nbest_ref.py) and the reference's own rankings, through the C ABI, the engine binding and the
plugin (GPU).

The explicit selection has to return the restatement's indices exactly.  On the hot path every entry is rebuilt from
its own float32 loss in Python doubles (the score must carry those bits) and compared with the reference's final_score of
the same candidate within 2e-3 -- what a float32 device loss may move a final score by (test_gpu_postlogits.py).  Rank
positions are compared wherever the reference itself separates them: a rank whose reference neighbours are both more than
2e-3 away, or exact ties of one token list scored under two keys (one loss on the device as well), has to hold the
reference's candidate; ranks in a near-tie group are compared as sets.  Where only the reference's first 20 are recorded,
the neighbour below the last of them is the device's next entry, with twice the margin (its own error plus the gap).
By the reference's own neighbours 53 of the 1,370 ranks compared are near ties (3.9 %, 41 of them at text_weight = -0.5
with no span penalty); with the last recorded ranks whose lower neighbour turned out near on the device it is 59 (4.3 %).
The test holds the share to 5 %."""

import gzip
import json
import math
import struct

import numpy as np
import pytest
import torch

import knob_cases as kc
import nbest_ref
from nbest_ref import MARGIN
from synth import synth_audio, synth_logits

pytestmark = pytest.mark.gpu

FORCE_CTC = math.nextafter(1.0, 2.0)      # no text score reaches it: the gate fails for every utterance
K = 20
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048]
HOT_RUNS = [(s, f) for s in ("e2e", "K3", "K5", "K6") for f in (False, True)]


@pytest.fixture(scope="module")
def engine():
    from offline_tarteel_amd.engine import Engine

    eng = Engine(device=0, with_model=False, max_batch=32)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def data(golden_dir):
    d = kc.load(golden_dir)
    d["e2e"] = json.load(gzip.open(golden_dir / "e2e_cases.json.gz"))
    return d


def make_engine(**kw):
    from offline_tarteel_amd.engine import Engine

    return Engine(device=0, with_model=False, max_batch=32, **kw)


def ragged(lps):
    t_max = max(x.shape[0] for x in lps)
    batch = torch.full((len(lps), t_max, 1025), -50.0)
    for b, x in enumerate(lps):
        batch[b, : x.shape[0]] = x
    assert t_max <= 376 and len(lps) <= 32
    return batch.cuda().contiguous(), [x.shape[0] for x in lps]


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------ 1. the selection itself
def value_rows(n, seed):
    """(name, finals, losses) for one size: what the selection can get wrong"""
    rng = np.random.default_rng(seed)
    ok = np.ones(n, np.float32)
    distinct = rng.standard_normal(n)
    coarse = rng.integers(0, 8, n).astype(np.float64) / 4.0 - 1.0          # 8 levels: ties everywhere, index order decides
    holes = np.where(rng.random(n) < 0.5, np.float32(np.inf), np.float32(2.5)).astype(np.float32)
    if n > 2:
        holes[1], holes[2] = -np.inf, np.nan                                # not finite either
    rows = [("distinct", distinct, ok), ("coarse", coarse, ok), ("equal", np.full(n, -3.25), ok),
            ("holes", distinct, holes), ("coarse-holes", coarse, holes), ("all-inf", distinct, np.full(n, np.inf, np.float32)),
            ("zeros", np.where(rng.random(n) < 0.5, 0.0, -0.0), ok),
            ("zeros-and-ones", rng.choice(np.array([0.0, -0.0, -1.0, 1.0]), n), ok)]
    for name, pos in (("max-at-0", 0), ("max-at-255", 255), ("max-at-256", 256), ("max-at-last", n - 1)):
        if 0 <= pos < n:
            v = coarse.copy()
            v[pos] = 10.0
            rows.append((name, v, ok))
    return rows


@pytest.mark.parametrize("k", [1, 5, 32])
def test_select_equals_the_restatement(engine, k):
    """every size around the wave, block and capacity edges, every value pattern: the indices are the restatement's; the
    rows of one ragged call carry what their own single-row calls return"""
    per_size = {n: value_rows(n, 1000 + n) for n in SIZES}
    names = [r[0] for r in per_size[2048]]
    checked = 0
    for name in names:
        rows = [(n, next((r for r in per_size[n] if r[0] == name), None)) for n in SIZES]
        rows = [(n, r) for n, r in rows if r is not None]
        finals, losses = [r[1] for _, r in rows], [r[2] for _, r in rows]
        together = engine.nbest_select(finals, losses, k)
        for (n, _), f, l, got in zip(rows, finals, losses, together):
            want = nbest_ref.select(f.tolist(), l.tolist(), k)
            assert got == want, (name, n, k, got[:8], want[:8])
            assert engine.nbest_select([f], [l], k)[0] == got, (name, n, k)
            checked += 1
    assert checked >= 8 * len(SIZES)
    # the patterns do what they are there for
    f, l = per_size[2048][1][1], per_size[2048][1][2]
    top = nbest_ref.select(f.tolist(), l.tolist(), 32)
    assert len(set(f[top])) == 1 and top == sorted(top)                    # coarse: one level, in index order
    z = per_size[257][6][1]
    assert np.signbit(z).any() and not np.signbit(z).all() and nbest_ref.select(z.tolist(), [0.0] * 257, 5) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------ 2. the hot path against the reference
def reference_ranking(c, tb):
    """(candidate keys in list order, [(candidate index, reference final)] best first over the first 2,048 candidates,
    whether that is the WHOLE ranking, text scores or None)"""
    if "keys" in c:
        keys, scores, kn = c["keys"], c["scores"], c["knobs"]
    else:
        keys, scores, kn = c["cand_keys"], None, kc.DEFAULTS
    if "rerank" in c:
        fin = c["rerank"]["final_score"][: kc.CAND_CAP]
    elif "ctc_loss" in c:
        fin = [None if l is None else nbest_ref.reference_final(l, n, 0.0, k[2] - k[1] + 1, kn["text_weight"], kn["span_penalty"])
               for l, n, k in zip(c["ctc_loss"], c["ctc_len"], keys)]
    else:
        pos = {tuple(k): i for i, k in enumerate(keys)}
        head = [(pos[tuple(k)], f) for k, f in zip(c["ranked_keys"], c["ranked_final"]) if pos[tuple(k)] < kc.CAND_CAP]
        return keys, head, len(c["ranked_keys"]) < 20 and len(keys) <= kc.CAND_CAP, scores
    return keys, [(i, fin[i]) for i in nbest_ref.rank(fin)], True, scores


def check_ctc_row(c, r, info, ent, ent32, tb, tally):
    tag = (c.get("set", "e2e"), c["name"])
    keys, ref, complete, scores = reference_ranking(c, tb)
    kn = c.get("knobs", kc.DEFAULTS)
    n = int(info["n_entries"])
    if complete:
        assert n == min(K, len(ref)) and int(info["n_ranked"]) == len(ref), (tag, n, int(info["n_ranked"]), len(ref))
    else:
        assert n == K and int(info["n_ranked"]) >= K and len(ref) == K, (tag, n, len(ref))
    assert int(info["source"]) == 2 and int(info["flags"]) == r["flags"] and r["source"] == "ctc", tag
    e = ent[:n]
    assert ent[n:].tobytes() == bytes(ent[n:].nbytes), tag
    assert e.tobytes() == ent32[:n].tobytes(), tag                          # k = 20 is the head of k = 32
    # entry 0 is the prediction
    assert (int(e[0]["surah"]), int(e[0]["ayah"]), int(e[0]["ayah_end"])) == (r["surah"], r["ayah"], r["ayah_end"]), tag
    assert bits(e[0]["ctc_norm_loss"]) == bits(r["ctc_norm_loss"]), tag
    ref_final = dict(ref)
    for x in e:
        ci, st, sp = int(x["cand_index"]), int(x["start_verse"]), int(x["span"])
        key = [int(x["surah"]), int(x["ayah"]), int(x["ayah_end"])]
        assert key == keys[ci] == list(tb.key_of(st, sp)) and int(x["source"]) == 2, (tag, ci)
        L = len(tb.token_ids(st, sp))
        assert int(x["n_tokens"]) == L and math.isfinite(float(x["ctc_loss"])), (tag, ci)
        norm = np.float32(x["ctc_loss"]) / np.float32(L)
        assert bits(x["ctc_norm_loss"]) == bits(norm), (tag, ci)
        # run.py:376 in Python doubles from the entry's own loss: the score carries exactly those bits
        assert float(x["score"]) == -float(norm) + kn["text_weight"] * float(x["text_score"]) - kn["span_penalty"] * (sp - 1), (tag, ci)
        if scores is not None:
            assert float(x["text_score"]) == scores[ci], (tag, ci)
        if ci in ref_final:
            print(f"{tag} cand {ci}: device {float(x['score']):.6f} reference {ref_final[ci]:.6f}")
            assert abs(float(x["score"]) - ref_final[ci]) <= MARGIN, (tag, ci, float(x["score"]), ref_final[ci])
        else:       # outside the recorded head: it cannot beat the reference's last recorded rank by more than the margin
            assert not complete and float(x["score"]) <= ref[-1][1] + MARGIN, (tag, ci)
    order = [(-float(x["score"]), int(x["cand_index"])) for x in e]
    assert all(a < b for a, b in zip(order, order[1:])), tag
    # rank positions
    def toks(i):
        s, a, e = keys[ref[i][0]]
        return tb.token_ids(tb.verse_index(s, a), e - a + 1).tolist()

    finals = [f for _, f in ref]
    groups = nbest_ref.tie_groups(finals, lambda i, j: toks(i) == toks(j))
    open_last = False
    if not complete:     # the neighbour below the recorded head is the device's next entry
        assert len(ent32) > K
        nxt = ent32[K]
        open_last = int(nxt["source"]) == 2 and finals[-1] - float(nxt["score"]) <= 2 * MARGIN
    dev = [int(x["cand_index"]) for x in e]
    for g in sorted(set(groups[:n])):
        ranks = [i for i, gg in enumerate(groups) if gg == g]
        inside = [i for i in ranks if i < n]
        closed = len(inside) == len(ranks) and not (open_last and ranks[-1] == len(ref) - 1)
        members = [ref[i][0] for i in ranks]
        got = [dev[i] for i in inside]
        if len(ranks) == 1 and closed:
            assert got == members, (tag, "rank", ranks[0], got, members)
            tally["strict"] += 1
            continue
        tally["near"] += len(inside)
        if closed:
            assert sorted(got) == sorted(members), (tag, "ranks", ranks, got, members)
        else:
            low = min(finals[i] for i in ranks)
            for i in inside:
                assert dev[i] in members or abs(float(e[i]["score"]) - low) <= 2 * MARGIN, (tag, "rank", i, dev[i], members)


def check_text_row(c, r, info, ent, reranked):
    tag = (c.get("set", "e2e"), c["name"])
    b = c["base"]
    assert (int(info["n_entries"]), int(info["n_ranked"]), int(info["source"])) == (1, 0, 1), (tag, info)
    assert bool(int(info["flags"]) & 4) == reranked and int(info["flags"]) == r["flags"], tag
    x = ent[0]
    assert [int(x["surah"]), int(x["ayah"]), int(x["ayah_end"])] == [b[0], b[1], b[2] or b[1]] == [r["surah"], r["ayah"], r["ayah_end"]], tag
    assert float(x["score"]) == float(x["text_score"]) == b[3] == r["base_score"] == r["score"], tag
    assert (int(x["cand_index"]), int(x["source"]), int(x["n_tokens"]), float(x["ctc_loss"])) == (-1, 1, 0, 0.0), tag
    assert int(x["span"]) == (b[2] or b[1]) - b[1] + 1
    assert ent[1:].tobytes() == bytes(ent[1:].nbytes), tag
    assert r["nbest"][0]["source"] == "text" and len(r["nbest"]) == 1


@pytest.fixture(scope="module")
def hot(data):
    """one ragged batch per (fixture set, own threshold | every row reranks), made and judged on first use"""
    done = {}

    def run(set_name, forced, wide=False):
        key = (set_name, forced, wide)
        if key in done:
            return done[key]
        cases = data["e2e"] if set_name == "e2e" else kc.cases_of(data, set_name)
        knobs = dict(kc.DEFAULTS if set_name == "e2e" else data["sets"][set_name])
        if forced:
            knobs["threshold"] = FORCE_CTC
        eng = make_engine(max_transcript=2048 if wide else 1024, **knobs)
        try:
            dev, Ts = ragged([kc.lp_of(c["recipe"]) for c in cases])
            rows = eng.decode_retrieve_rerank(dev, Ts, nbest=K)
            info, ent = eng.nbest_raw(batch=len(cases), k=K)
            _, ent32 = eng.nbest_raw(batch=len(cases), k=32)
            plain = eng.decode_retrieve_rerank(dev, Ts)
            tally = {"strict": 0, "near": 0, "ctc": 0, "text": 0, "none": 0}
            for b, (c, r) in enumerate(zip(cases, rows)):
                assert {k: v for k, v in r.items() if k != "nbest"} == plain[b], c["name"]    # the prediction itself is untouched
                assert len(r["nbest"]) == int(info[b]["n_entries"])
                assert [x["cand_index"] for x in r["nbest"]] == ent[b, : len(r["nbest"])]["cand_index"].tolist()
                if "base" not in c:
                    assert (int(info[b]["n_entries"]), int(info[b]["source"])) == (0, 0) and r["nbest"] == [] and not r["surah"]
                    assert ent[b].tobytes() == bytes(ent[b].nbytes)
                    tally["none"] += 1
                    continue
                reranked = forced or c["use_ctc"]
                assert r["use_ctc"] == reranked, c["name"]
                if reranked and reference_ranking(c, eng.tables)[1]:
                    check_ctc_row(c, r, info[b], ent[b], ent32[b], eng.tables, tally)
                    tally["ctc"] += 1
                else:
                    check_text_row(c, r, info[b], ent[b], reranked)
                    tally["text"] += 1
            if set_name == "e2e":   # the fixture records no text scores: the retrieval's own, pinned by test_gpu_postlogits.py
                for b, c in enumerate(cases):
                    if int(info[b]["source"]) == 2:
                        sc = eng.debug_retrieve(c["transcript"])["cand_score"]
                        for x in ent[b, : int(info[b]["n_entries"])]:
                            assert float(x["text_score"]) == sc[int(x["cand_index"])], c["name"]
        finally:
            eng.close()
        done[key] = {"tally": tally, "info": info.copy(), "ent": ent.copy(), "names": [c["name"] for c in cases]}
        return done[key]

    return run


@pytest.mark.parametrize("set_name,forced", HOT_RUNS, ids=[s + ("-forced" if f else "") for s, f in HOT_RUNS])
def test_hot_path_lists_against_the_reference(hot, set_name, forced):
    got = hot(set_name, forced)
    t = got["tally"]
    print(set_name, forced, t)
    assert t["ctc"] >= (6 if forced else 5) and t["strict"] > 0
    if forced:
        # noise_only: reranked, nothing feasible -> the text base with n_ranked = 0
        b = got["names"].index("noise_only")
        assert (int(got["info"][b]["source"]), int(got["info"][b]["n_ranked"]), int(got["info"][b]["n_entries"])) == (1, 0, 1)
        assert int(got["info"][b]["flags"]) & 4
    else:
        assert t["text"] >= 2          # gate-pass rows: [base]


def test_near_tie_share_of_the_compared_ranks(hot):
    strict = near = 0
    for set_name, forced in HOT_RUNS:
        t = hot(set_name, forced)["tally"]
        strict += t["strict"]
        near += t["near"]
    print(f"ranks compared {strict + near}, in near-tie groups {near} ({100.0 * near / (strict + near):.1f} %)")
    assert strict + near >= 1300
    assert near <= 0.05 * (strict + near), (near, strict)


# ------------------------------------------------------------------ 4. the wide kernel set
def test_wide_kernel_set_gives_the_same_lists(hot):
    a, b = hot("K5", False), hot("K5", False, wide=True)
    assert a["info"].tobytes() == b["info"].tobytes() and a["ent"].tobytes() == b["ent"].tobytes()
    assert (a["info"]["flags"] & 8).any()       # clipped lists among them


# ------------------------------------------------------------------ 3. runners-up of the text match
def segment(tb, text):
    """fewest vocabulary pieces whose surfaces spell `text` (what the greedy decode of their frames turns back into it)"""
    target = " " + text
    by_first = {}
    for i in range(1, 1024):
        s = tb.piece_surface[i]
        if s:
            by_first.setdefault(s[0], []).append((s, i))
    n = len(target)
    best = [None] * (n + 1)
    best[0] = (0, None, None)
    for p in range(n):
        if best[p] is None:
            continue
        for s, i in by_first.get(target[p], ()):
            q = p + len(s)
            if target.startswith(s, p) and (best[q] is None or best[q][0] > best[p][0] + 1):
                best[q] = (best[p][0] + 1, p, i)
    if best[n] is None:
        return None
    ids, p = [], n
    while p:
        _, p0, i = best[p]
        ids.append(i)
        p = p0
    return ids[::-1]


def test_runners_follow_the_base_on_gate_pass_rows(engine, golden_dir):
    from oracle.oracle import normalize_arabic

    tb = engine.tables
    cases, lps = [], []
    for c in json.load(gzip.open(golden_dir / "retrieval_cases.json.gz")):
        t = c["transcript"]
        if normalize_arabic(t) != t or c["match"]["score"] < 0.8:
            continue
        ids = segment(tb, t)
        if ids is None or 2 * len(ids) > 376:
            continue
        lps.append(torch.log_softmax(torch.from_numpy(synth_logits(ids, 2 * len(ids), seed=len(cases), noise=0.5, boost=12.0, rep=1)), -1))
        cases.append(c)
    assert len(cases) >= 12 and any(c["match"]["ayah_end"] for c in cases)
    dev, Ts = ragged(lps)
    rows = engine.decode_retrieve_rerank(dev, Ts)
    with_runners = engine.nbest_results(batch=len(cases), k=32, runners=True)
    short = engine.nbest_results(batch=len(cases), k=3, runners=True)
    without = engine.nbest_results(batch=len(cases), k=32)
    for c, r, lst, s3, one in zip(cases, rows, with_runners, short, without):
        assert r["transcript"] == c["transcript"] and not r["use_ctc"] and r["source"] == "text", c["name"]
        d = engine.debug_retrieve(c["transcript"])            # (reuses the context: after the n-best calls)
        want = nbest_ref.text_row(d["base_start"], d["base_span"], d["base_score"], d["runner_idx"], d["runner_score"], k=32, runners=True)
        assert [(x["start"], x["span"], x["score"]) for x in lst] == [(w["start"], w["span"], w["score"]) for w in want], c["name"]
        assert len(lst) == 32 and s3 == lst[:3] and one == lst[:1], c["name"]
        assert lst[0]["score"] == r["score"] == c["match"]["score"] and (lst[0]["surah"], lst[0]["ayah"], lst[0]["ayah_end"]) == (
            r["surah"], r["ayah"], r["ayah_end"]), c["name"]
        assert all(x["source"] == "text" and x["cand_index"] == -1 and x["span"] == 1 and x["text_score"] == x["score"] for x in lst[1:])
        assert (lst[0]["start"], lst[0]["span"]) not in {(x["start"], x["span"]) for x in lst[1:]}, c["name"]
        # the fixture's runners_up (rounded to 3 places; a single-verse base leads that list, a span does not appear in it)
        g = c["match"]["runners_up"]
        mine = [[x["surah"], x["ayah"], round(x["score"], 3)] for x in (lst if d["base_span"] == 1 else lst[1:])]
        assert mine == g[: len(mine)], c["name"]


# ------------------------------------------------------------------ 5. context ownership
def test_nbest_belongs_to_its_context():
    """two contexts, two batches in flight: the list of context 0 asked for AFTER the second launch is the first batch's.
    Seeded random weights recognise nothing, so the post-logits stages read injected verse-shaped log-probs, a different
    tensor per batch (the pattern of test_gpu_align.py)."""
    from offline_tarteel_amd.engine import Engine, QvError

    eng = Engine(device=0, with_model=True, seed=7, max_batch=2, max_samples=32000, contexts=2, threshold=FORCE_CTC)
    try:
        tb = eng.tables
        T = 24

        def verse_lp(refs, seed):
            rows = []
            for k, (s, a) in enumerate(refs):
                ids = tb.token_ids(tb.verse_index(s, a), 1).tolist()
                assert 2 * len(ids) <= T
                rows.append(torch.log_softmax(torch.from_numpy(synth_logits(ids, T, seed=seed + k, noise=1.0, boost=8.0, rep=1)), -1))
            return torch.stack(rows)

        dev_a = verse_lp([(112, 2), (112, 1)], 1).cuda().contiguous()
        dev_b = verse_lp([(112, 3), (112, 4)], 5).cuda().contiguous()
        audio = torch.from_numpy(synth_audio(2, 32000)).cuda()
        lens = [32000, 32000]
        eng.inject_logprobs(dev_a, [T, T])
        ctx0 = eng.predict_batch_async(audio, lens)
        eng.inject_logprobs(dev_b, [T, T])
        ctx1 = eng.predict_batch_async(audio, lens)
        assert ctx0 != ctx1
        nb0 = eng.nbest_results(ctx0, 2, k=5)
        res0 = eng.fetch_results(ctx0, 2, T)
        nb1 = eng.nbest_results(ctx1, 2, k=5)
        res1 = eng.fetch_results(ctx1, 2, T)
        eng.inject_logprobs(None)
        keys0 = [(r["surah"], r["ayah"]) for r in res0]
        keys1 = [(r["surah"], r["ayah"]) for r in res1]
        assert all(k[0] for k in keys0 + keys1) and not set(keys0) & set(keys1), (keys0, keys1)
        for nb, res in ((nb0, res0), (nb1, res1)):
            for b in range(2):
                assert res[b]["source"] == "ctc" and 1 <= len(nb[b]) <= 5
                assert (nb[b][0]["surah"], nb[b][0]["ayah"], nb[b][0]["ayah_end"]) == (res[b]["surah"], res[b]["ayah"], res[b]["ayah_end"])
                assert bits(nb[b][0]["ctc_norm_loss"]) == bits(res[b]["ctc_norm_loss"])
        # nothing to list once the context's workspace has been reused by a single-text call
        eng.match_verse("قل هو الله احد")
        with pytest.raises(QvError):
            eng.nbest_results(int(eng.lib.qv_last_context(eng.h)), 2)
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. argument errors and the plugin
def test_argument_errors(data):
    import ctypes as C

    from offline_tarteel_amd.engine import NBEST_ENTRY_DTYPE, NBEST_INFO_DTYPE, QvError

    eng = make_engine()
    try:
        info, ent = np.zeros(33, NBEST_INFO_DTYPE), np.zeros((33, 32), NBEST_ENTRY_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

        def results(ctx=0, batch=1, k=5, flags=0, i=info, e=ent):
            return eng.lib.qv_nbest_results_ctx(eng.h, ctx, batch, k, flags, p(i) if i is not None else None, p(e) if e is not None else None)

        assert results() == 1                               # QV_ERR_ARG: the context holds no batch yet
        dev, Ts = ragged([kc.lp_of(c["recipe"]) for c in data["e2e"][:3]])
        eng.decode_retrieve_rerank(dev, Ts)
        assert results(batch=3) == 0 and results(batch=3, k=1) == 0 and results(batch=3, k=32, flags=1) == 0
        for bad in (dict(k=0), dict(k=33), dict(k=-1), dict(flags=2), dict(flags=-1), dict(ctx=-1), dict(ctx=1), dict(batch=0),
                    dict(batch=4), dict(i=None), dict(e=None)):          # batch=4: more than the context's batch of 3
            assert results(**bad) == 1, bad
        assert results(batch=33) == 4                       # QV_ERR_CAPACITY
        with pytest.raises(QvError):
            eng.nbest_results(batch=3, k=33)
        fin, los, n = np.zeros((33, 8)), np.zeros((33, 8), np.float32), np.full(33, 8, np.int32)
        idx, cnt = np.zeros((33, 32), np.int32), np.zeros(33, np.int32)

        def select(rows=2, pitch=8, k=5, f=fin, nn=n):
            return eng.lib.qv_nbest_select(eng.h, p(f) if f is not None else None, p(los), p(nn), rows, pitch, k, p(idx), p(cnt), None)

        assert select() == 0 and cnt[:2].tolist() == [5, 5] and idx[0, :5].tolist() == [0, 1, 2, 3, 4]
        for bad in (dict(rows=0), dict(pitch=0), dict(pitch=2049), dict(k=0), dict(k=33), dict(f=None),
                    dict(nn=np.full(33, 9, np.int32)), dict(nn=np.full(33, -1, np.int32))):
            assert select(**bad) == 1, bad
        assert select(rows=33) == 4
        # the explicit form leaves the context's batch alone
        assert results(batch=3) == 0
    finally:
        eng.close()


def test_plugin_candidates(tmp_path, monkeypatch):
    """predict_batch(paths, candidates=5) on the small synthetic WAV corpus of the plugin tests: [] where nothing is
    recognised (seeded random weights), well-formed lists where a verse is (injected verse-shaped log-probs); without
    candidates= the dicts are the same as before"""
    from offline_tarteel_amd import plugin

    paths = []
    for i, n in enumerate((24000, 36000, 30000)):
        data = (synth_audio(1, n, seed=50 + i)[0] * 20000).astype("<i2").tobytes()
        hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack(
            "<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", len(data))
        (tmp_path / f"s{i}.wav").write_bytes(hdr + data)
        paths.append(str(tmp_path / f"s{i}.wav"))
    monkeypatch.setenv("QVERSE_RANDOM_WEIGHTS", "1")
    monkeypatch.setattr(plugin, "_engine", None)
    monkeypatch.setattr(plugin, "MAX_SAMPLES", 64000)
    monkeypatch.setattr(plugin, "MAX_BATCH", 4)
    try:
        plain = plugin.predict_batch(paths)
        with_c = plugin.predict_batch(paths, candidates=5)
        for a, b in zip(plain, with_c):
            assert {k: v for k, v in b.items() if k != "candidates"} == {k: v for k, v in a.items() if k != "candidates"}
            assert ("candidates" in a) == (not a["surah"])       # (the empty prediction always carried the key)
            if not a["surah"]:
                assert b["candidates"] == []
        eng = plugin._engine
        tb = eng.tables
        T = 24
        refs = [(112, 2), (112, 1), (112, 3)]
        lp = torch.stack([torch.log_softmax(torch.from_numpy(synth_logits(
            tb.token_ids(tb.verse_index(s, a), 1).tolist(), T, seed=9 + k, noise=1.0, boost=8.0, rep=1)), -1)
            for k, (s, a) in enumerate(refs)]).cuda().contiguous()
        eng.inject_logprobs(lp, [T] * 3)
        seen = plugin.predict_batch(paths, candidates=5)
        both = plugin.predict_batch(paths, words=True, candidates=5)
        monkeypatch.setattr(plugin, "_CANDIDATES", 5)
        one = plugin.predict(paths[1])          # (a clip with at least T frames; a batch of one reads injected row 0)
        eng.inject_logprobs(None)
        assert one["candidates"] == seen[0]["candidates"]
        assert any(d["surah"] for d in seen)
        for d, w in zip(seen, both):
            assert w["candidates"] == d["candidates"] and "words" in w
            if not d["surah"]:
                assert d["candidates"] == []
                continue
            cands = d["candidates"]
            assert 1 <= len(cands) <= 5 and all(set(x) == {"surah", "ayah", "ayah_end", "score"} for x in cands)
            assert (cands[0]["surah"], cands[0]["ayah"], cands[0]["ayah_end"]) == (d["surah"], d["ayah"], d["ayah_end"])
            assert all(x["score"] == round(x["score"], 4) and 1 <= x["surah"] <= 114 and x["ayah"] <= x["ayah_end"] for x in cands)
            if d["source"] == "text":
                assert cands == [{"surah": d["surah"], "ayah": d["ayah"], "ayah_end": d["ayah_end"], "score": d["score"]}]
            else:
                assert all(a["score"] >= b["score"] for a, b in zip(cands, cands[1:]))
    finally:
        if plugin._engine is not None:
            plugin._engine.close()
        monkeypatch.setattr(plugin, "_engine", None)
