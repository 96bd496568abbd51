"""Inputs for the tests of the decode stage (csrc/qv_postlogits.hip, k_decode): pure numpy builders, no GPU and no kernel.

A case is (name, log-probs float32 [T, 1025], T).  Ordinary frames are hash_noise plus 12 on the intended id through a
float32 log-softmax -- the noise is bounded by 3.45, so the boost decides every frame (tests/test_gpu_long_transcript.py,
dense_logprobs).  Tie frames are literal float32 values: a log-softmax would not keep two entries equal.

The reference of every case is numpy and the oracle (reference_of): Oracle.greedy_ids for the ids,
normalize_arabic(ids_to_text(ids).strip()) for the text, the table's encode for the codes, len(text.split()) for the
words.  decode_host() is a numpy restatement of what the kernel does (per-frame first maximum, collapse in chunks of 64
frames, per-piece code expansion, whitespace collapse and strip); tests/test_decode_host.py holds it to the reference on
every case and shows with two deliberately wrong variants that the cases tell them apart."""

from __future__ import annotations

import numpy as np

from synth import BLANK, VOCAB, hash_noise

BOOST = np.float32(12.0)
NOISE_BOUND = 3.45            # |hash_noise| <= 510 / 147.8
RAW_CAP = 4096                # csrc/qv_common.h QV_RAW_CAP: raw (pre-collapse) code units per utterance
EMPTY_PIECES = (16, 20, 23, 27, 30, 56, 62, 80, 85, 107, 129, 134, 202, 235, 288)   # normalise to nothing
UNK, SPACE = 0, 10            # ' ⁇ ' (space, a character outside the alphabet, space) and a lone ' '
T_FULL = 768                  # frames of an engine created for 979,200 samples, +2: the full row capacity
MAX_SAMPLES = 979200
T_TEXT_MAX = 766              # qv_frames_for_samples(979200): the long texts fit in this many frames


# ------------------------------------------------------------------ the vocabulary ---------------------------------------

class Pieces:
    """per-id normalised code strings of the static table (what the kernel expands from), read on the host"""

    def __init__(self, oracle):
        off, codes = oracle.t["piece_off"], oracle.t["piece_codes"]
        self.codes = [np.asarray(codes[int(off[i]): int(off[i + 1])], np.uint8) for i in range(VOCAB)]
        self.len = np.array([len(c) for c in self.codes])
        # one-code pieces that are a letter of the alphabet: they move the raw position by exactly one
        self.fillers = [i for i in range(1024) if self.len[i] == 1 and 0 < self.codes[i][0] < 40]
        # leading-space pieces, longest first (ties: smaller id)
        self.spaced = sorted((i for i in range(1024) if self.len[i] >= 2 and self.codes[i][0] == 0 and i not in (UNK, SPACE)),
                             key=lambda i: (-self.len[i], i))

    def raw(self, ids) -> np.ndarray:
        """the raw (pre-collapse) code units of a token list: the pieces' codes back to back"""
        return np.concatenate([self.codes[int(i)] for i in ids] + [np.zeros(0, np.uint8)])


# ------------------------------------------------------------------ frames -----------------------------------------------

def log_softmax32(lg: np.ndarray) -> np.ndarray:
    x = lg.astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def frames_of(frame_ids, seed: int) -> np.ndarray:
    """float32 [T, 1025] log-probs whose per-frame argmax is frame_ids (BLANK = 1024 for a blank frame)"""
    p = np.asarray(frame_ids, np.int64).reshape(-1)
    T = len(p)
    lg = hash_noise((T, VOCAB), seed)
    lg[np.arange(T), p] += BOOST
    return np.ascontiguousarray(log_softmax32(lg))


def path_of(ids) -> list[int]:
    """one frame per token, a blank ONLY between equal neighbours (CTC needs no other)"""
    path = []
    for tok in ids:
        if path and path[-1] == int(tok):
            path.append(BLANK)
        path.append(int(tok))
    return path


def base_frame(seed: int) -> np.ndarray:
    """a literal frame whose every entry is clearly negative (noise - 20): the canvas of the tie frames"""
    return (hash_noise((VOCAB,), seed) - np.float32(20.0)).astype(np.float32)


def tie_frame(indices, seed: int, value: float = -1.0) -> np.ndarray:
    f = base_frame(seed)
    f[list(indices)] = np.float32(value)
    return f


# (tied indices, the winner numpy's first-maximum rule names).  The kernel scans lane + 64 i for i = 0..16 per lane and
# reduces over the lanes by xor: (5, 6) ties across lanes, (5, 69) across strides of one lane, (63, 64) the last lane of
# stride 0 against the first of stride 1, the blank at 1024 is lane 0's 17th stride.
TIES = [((5, 6), 5), ((5, 69), 5), ((63, 64), 63), ((6, 70, 134), 6), ((0, 1024), 0), ((1023, 1024), 1023), ((960, 1024), 960)]
UNIQUE_MAXIMA = [0, 63, 64, 1023, 1024] + [64 * k + j for k in range(16) for j in (0, 63)]


def argmax_frames():
    """[(tag, frame float32 [1025], expected index)] -- every expectation is np.argmax of the same array (asserted on the
    host), written out here so that the intended winner is on record"""
    out = []
    for n, i in enumerate(UNIQUE_MAXIMA):
        out.append((f"unique {i}", frames_of([i], 700 + n)[0], i))
    for n, (idx, win) in enumerate(TIES):
        out.append((f"tie {idx}", tie_frame(idx, 800 + n), win))
    out.append(("all equal", np.full(VOCAB, np.float32(-6.9324), np.float32), 0))
    f = base_frame(820)
    f[3], f[700] = np.float32(-0.0), np.float32(0.0)
    out.append(("-0.0 at 3, +0.0 at 700", f, 3))
    f = base_frame(821)
    f[3], f[2] = np.float32(0.0), np.float32(-0.0)
    out.append(("+0.0 at 3, -0.0 at 2", f, 2))
    return out


def spaced_rows(frames, seed: int) -> np.ndarray:
    """the frames in order with one ordinary blank frame between neighbours: equal winners of consecutive frames stay
    two tokens, so the collapsed ids show every frame's winner"""
    rows = []
    for n, f in enumerate(frames):
        if n:
            rows.append(frames_of([BLANK], seed + n)[0])
        rows.append(f)
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32)


# ------------------------------------------------------------------ id lists ---------------------------------------------

def text_ids(pc: Pieces, n_chars: int):
    """token ids whose normalised text has exactly n_chars characters, from the two longest leading-space pieces
    alternating (no blank between different ids) and one-code fillers at the end"""
    a, b = pc.spaced[0], pc.spaced[1]
    f1, f2 = pc.fillers[0], pc.fillers[1]
    ids, n = [], -1                                  # the first piece's leading space is stripped
    while n + int(pc.len[(a, b)[len(ids) % 2]]) + 2 <= n_chars:
        p = (a, b)[len(ids) % 2]
        ids.append(p)
        n += int(pc.len[p])
    # the last word: a shorter leading-space piece, then one-code pieces up to the exact length
    tail = next(i for i in pc.spaced if pc.len[i] <= n_chars - n and i not in (a, b))
    ids.append(tail)
    n += int(pc.len[tail])
    while n < n_chars:
        ids.append(f1 if ids[-1] != f1 else f2)
        n += 1
    return ids


def straddle_ids(pc: Pieces):
    """runs of two and three spaces across raw positions 63|64 and 127|128, steered there by one-code fillers"""
    f1, f2 = pc.fillers[0], pc.fillers[1]
    sp = pc.spaced[-1]                                # a short leading-space piece
    ids = []

    def fill_to(pos):
        while len(pc.raw(ids)) < pos:
            ids.append(f1 if not ids or ids[-1] != f1 else f2)

    fill_to(63)
    ids.extend([SPACE, sp])                           # raw 63 = ' ' (id 10), raw 64 = the piece's own leading space
    fill_to(126)
    ids.extend([SPACE, SPACE, sp])                    # raw 126, 127 = ' ' ' ', raw 128 = the piece's leading space
    ids.extend([f1, f2])
    return ids


def build_cases(oracle):
    """[(name, log-probs [T, 1025] float32, T)] -- built once per test module and never modified"""
    pc = Pieces(oracle)
    f1, f2, f3 = pc.fillers[:3]
    sp = pc.spaced[-1]
    cases = []

    def add(name, lp):
        lp = np.ascontiguousarray(lp, np.float32).reshape(-1, VOCAB)
        lp.setflags(write=False)
        cases.append((name, lp, lp.shape[0]))

    def add_ids(name, ids, seed):
        add(name, frames_of(path_of(ids), seed))

    # --- argmax
    am = argmax_frames()
    add("argmax unique", np.stack([f for tag, f, _ in am if tag.startswith("unique")]))
    add("argmax ties", spaced_rows([f for tag, f, _ in am if not tag.startswith("unique")], 830))
    one = np.full(VOCAB, -np.inf, np.float32)
    one[f3] = np.float32(-0.25)
    add("-inf but one", one)                          # (T = 1: no CTC target fits, the rerank's recursion never sees the row)
    add("-inf everywhere", np.full(VOCAB, -np.inf, np.float32))
    # --- collapse
    p = [BLANK] * 130
    p[60:67] = [f1] * 7
    p[125:130] = [f2] * 5
    add("merge across 63|64 and 127|128", frames_of(p, 840))
    for k, s in enumerate((62, 63)):
        p = [BLANK] * 131
        p[s], p[s + 2] = f1, f1
        p[s + 64], p[s + 66] = f2, f2
        p[0], p[130] = f3, f3
        add(f"id blank id from {s} and {s + 64}", frames_of(p, 841 + k))
    add("T=1 token", frames_of([f2], 843))
    add("T=1 blank", frames_of([BLANK], 844))
    add("T=0", np.zeros((0, VOCAB), np.float32))
    rng = np.random.default_rng(65)
    spoken = [i for i in range(1, 1024) if pc.len[i] > 0 and i != SPACE]
    for n in (65, 129):                               # n_tok crosses the 64-token expansion chunk once and twice
        ids = []
        while len(ids) < n:
            t = int(rng.choice(spoken))
            if not ids or t != ids[-1]:
                ids.append(t)
        add(f"{n} tokens", frames_of(ids, 845 + n))
    # one row of full capacity: a recitation at three frames per token, the last frame a token of its own
    verse = oracle.token_ids(oracle.verse_index(2, 282), 1).tolist()
    p = []
    for tok in verse:
        if p and p[-1] == tok:
            p.append(BLANK)
        p += [tok] * 3
    p = p[: T_FULL - 1]
    p.append(f1 if p[-1] != f1 else f2)
    assert len(p) == T_FULL
    add("T=768", frames_of(p, 848))
    # --- expansion and whitespace
    add_ids("only empty pieces", list(EMPTY_PIECES[:5]), 850)
    add_ids("only id 10", [SPACE], 851)
    add_ids("id 10 leading trailing doubled", [SPACE, f1, SPACE, SPACE, f2, sp, SPACE], 852)
    add_ids("id 0 start middle end doubled", [UNK, f1, UNK, f2, f3, UNK, UNK, f1, UNK], 853)
    add_ids("empty piece between letters", [f1, EMPTY_PIECES[0], f2, EMPTY_PIECES[7], EMPTY_PIECES[7], f3], 854)
    add_ids("leading-space piece after id 10", [f1, SPACE, sp, f2, SPACE, pc.spaced[0]], 855)
    add_ids("space runs across raw 63|64 and 127|128", straddle_ids(pc), 856)
    for n in (1024, 1025, 2048, 2049):
        add_ids(f"{n} characters", text_ids(pc, n), 860 + n)
    a, b = pc.spaced[0], pc.spaced[1]
    add_ids("raw overflow", [(a, b)[k % 2] for k in range(T_TEXT_MAX)], 870)
    return cases


LONG_TEXT_CASES = ("1024 characters", "1025 characters", "2048 characters", "2049 characters", "raw overflow", "T=768")


# ------------------------------------------------------------------ the reference ----------------------------------------

def reference_of(oracle, encode, lp: np.ndarray, T: int) -> dict:
    """ids, text, codes and word count of one case from numpy and the oracle"""
    from oracle.oracle import normalize_arabic

    ids = oracle.greedy_ids(lp[:T]) if T else []
    text = normalize_arabic(oracle.ids_to_text(ids).strip()) if ids else ""
    return {"ids": ids, "text": text, "codes": np.asarray(encode(text), np.uint8), "words": len(text.split())}


def expected_flags(ref: dict, pc: Pieces, window: int) -> int:
    """QV_FLAG_EMPTY_TRANSCRIPT (1) / QV_FLAG_TRANSCRIPT_TRUNCATED (2) as include/qverse.h documents them"""
    if len(pc.raw(ref["ids"])) > RAW_CAP or len(ref["text"]) > window:
        return 2
    return 1 if not ref["text"] else 0


# ------------------------------------------------------------------ the kernel's algorithm, restated on the host ---------

def argmax_first(frame: np.ndarray) -> int:
    """the kernel's scan: per lane the strides in ascending order with a strict >, then lanes merged with 'greater, or
    equal and smaller index'"""
    x = np.full(17 * 64, -np.inf, np.float32)
    x[:VOCAB] = frame
    best, bi = x[:64].copy(), np.arange(64)
    for i in range(1, 17):
        v = x[64 * i: 64 * i + 64]
        m = v > best
        best, bi = np.where(m, v, best), np.where(m, np.arange(64) + 64 * i, bi)
    w = 0
    for lane in range(1, 64):
        if best[lane] > best[w] or (best[lane] == best[w] and bi[lane] < bi[w]):
            w = lane
    return int(bi[w])


def argmax_last(frame: np.ndarray) -> int:
    """DELIBERATELY WRONG: the last maximum"""
    return int(VOCAB - 1 - np.argmax(frame[::-1]))


def decode_host(pc: Pieces, lp: np.ndarray, T: int, argmax=argmax_first, reset_prev_every: int = 0) -> dict:
    """reset_prev_every = 64 is the DELIBERATELY WRONG collapse that forgets the previous frame at every chunk start"""
    fid = [argmax(lp[t]) for t in range(T)]
    ids, prev = [], -1
    for t, i in enumerate(fid):
        if reset_prev_every and t % reset_prev_every == 0:
            prev = -1
        if i != prev and i != BLANK:
            ids.append(i)
        prev = i
    raw = pc.raw(ids)
    out = []
    nz = np.flatnonzero(raw)
    last = int(nz[-1]) if len(nz) else -1
    for i, c in enumerate(raw.tolist()):
        if c != 0 or (i > 0 and raw[i - 1] != 0 and i < last):
            out.append(c)
    codes = np.asarray(out, np.uint8)
    return {"ids": ids, "codes": codes, "words": int((codes == 0).sum()) + 1 if len(codes) else 0}


# ------------------------------------------------------------------ batches ----------------------------------------------

def batches_of(cases, size: int = 16):
    """ragged batches: the cases in order, `size` at a time"""
    return [cases[i: i + size] for i in range(0, len(cases), size)]


def batch_tensor(cases, pad: float = -50.0, t_max: int | None = None) -> tuple[np.ndarray, list[int]]:
    t_max = max(t_max or 1, max(T for _, _, T in cases))
    out = np.full((len(cases), t_max, VOCAB), np.float32(pad), np.float32)
    for b, (_, lp, T) in enumerate(cases):
        out[b, :T] = lp[:T]
    return out, [T for _, _, T in cases]
