"""Reference-side helpers for the length tests of the acoustic forward (tests/test_gpu_forward_lengths.py,
tests/test_forward_ref_host.py).  Everything here runs on the CPU with oracle/fastconformer_ref.py alone.

  * the twin (`F16Ops`): the fp32 restatement with the ONE rounding the device design chooses -- float16 operands of every
    Linear / Conv, float32 accumulation and bias.  Its distance `e` from the fp32 restatement is the reference-side floor
    the device is judged against: (a) device vs fp32 <= max(1e-2, FLOOR_K * e).  The device's distance from the twin --
    rule (b), "<= e" -- is printed and NOT asserted: measured, it is 0.58 - 1.04 e (0.6 - 1.13 e from the twin with the
    attention kernels' roundings), i.e. two f16-operand evaluations lie about as far from each other as from fp32.
  * `sharp_weights`: the seeded random weights with the attention's query side x4, on which the relative-position term
    is visible in the log-probs while `e` does not move.
  * two PLANTED reference errors (context managers): what a position off-by-one or a dropped last key frame in an
    attention kernel would compute.  A test whose bound such an oracle passes proves nothing about that error.
"""

from __future__ import annotations

import contextlib
import importlib.util
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

from oracle import fastconformer_ref as R
from ort_floor import FLOOR_K
from synth import synth_audio

ROOT = Path(__file__).resolve().parent.parent

LADDER = [1, 31, 32, 33, 64, 65, 127, 128, 129, 160, 255, 256, 257]   # the tile edges of test_frame_count_boundaries_are_batch_invariant
LADDER_AUDIO_SEED = 123
MAX_SAMPLES = 979200                          # 61 s: the longest clip qv_create accepts (766 encoder frames)
LONG = [766, 513, 417, 385, 377, 129]         # beyond 30 s (T = 376), around the 384-frame switch of the CTC / alignment kernels
LONG_AUDIO_SEED = 61
STRUCTURED_FRAMES = [38, 160, 417]
STRUCTURED_AUDIO_SEED = 5

SHARP_SUFFIXES = ("self_attn.linear_q.weight", "self_attn.linear_q.bias", "self_attn.pos_bias_u", "self_attn.pos_bias_v")


class F16Ops(R._Plain):
    """R.forward(..., ort=F16Ops()): inputs and weights of every linear / conv rounded through float16, fp32 accumulate,
    fp32 bias.  (With `ort` set R.forward runs every utterance alone and unpadded, and the CTC head as a 1x1 Conv.)"""

    def __init__(self):
        self._w16 = {}

    def _weight(self, w, name):
        t = w[name]
        hit = self._w16.get(name)
        if hit is None or hit[0] is not t:
            hit = (t, t.half().float())
            self._w16[name] = hit
        return hit[1]

    def linear(self, w, name, x, bias_name):
        return F.linear(x.half().float(), self._weight(w, name), w[bias_name] if bias_name else None)

    def conv(self, w, name, x, bias_name, fn, **kw):
        return fn(x.half().float(), self._weight(w, name), w[bias_name] if bias_name else None, **kw)


def sharp_weights(w: dict, gain: float = 4.0) -> dict:
    """"sharp attention": linear_q (weight and bias), pos_bias_u and pos_bias_v of every layer times `gain`, i.e. every
    attention logit -- content and position term alike -- times `gain`.  Nothing else changes."""
    out = dict(w)
    for name, t in w.items():
        if name.startswith("encoder.layers.") and name.endswith(SHARP_SUFFIXES):
            out[name] = (t * gain).contiguous()
    return out


def samples_for_frames(T):
    """smallest sample count whose three stride-2 stages leave exactly T encoder frames"""
    sl = lambda x: (x + 2 - 3) // 2 + 1  # noqa: E731
    n = 400
    while sl(sl(sl(n // 160 + 1))) < T:
        n += 160
    assert sl(sl(sl(n // 160 + 1))) == T
    return n


def clips(lens, seed: int) -> torch.Tensor:
    """synth_audio rows cut to `lens` samples (zero padded to the longest)"""
    a = torch.from_numpy(synth_audio(len(lens), max(lens), seed=seed))
    for b, n in enumerate(lens):
        a[b, n:] = 0
    return a


@contextlib.contextmanager
def positions_off_by_one():
    """planted error 1: the relative-position table rolled by one row (every query reads its neighbour's row)"""
    orig = R.rel_pos_emb
    R.rel_pos_emb = lambda T: torch.roll(orig(T), 1, 0)
    try:
        yield
    finally:
        R.rel_pos_emb = orig


@contextlib.contextmanager
def last_frame_dropped():
    """planted error 2: each utterance's last valid frame counts as padding in every layer (a partial last key tile cut
    one key short).  Compare all frames but the last."""
    orig = R.conformer_layer

    def layer(w, p, x, pos_emb, pad, *args, **kw):
        pad = pad.clone()
        last = (~pad).sum(1) - 1
        for b in range(pad.shape[0]):
            if int(last[b]) >= 0:
                pad[b, int(last[b])] = True
        return orig(w, p, x, pos_emb, pad, *args, **kw)

    R.conformer_layer = layer
    try:
        yield
    finally:
        R.conformer_layer = orig


def _h(x):
    return x.half().float()


def _layer_with_attention_roundings(w, p, x, pos_emb, pad, ops=None, taps=None, tag=""):
    """R.conformer_layer restated with the roundings the attention kernels perform on top of the f16 GEMM operands
    (csrc/qv_layers.hip: k_attention*): q, k, v and the projected position rows are STORED as float16, q + u and q + v are
    rounded to float16 MFMA operands, and exp(score - row max) is rounded to float16 before the P.V product while the row
    sum stays float32.  Everything outside the attention is R.conformer_layer's, line for line."""
    B, T, _ = x.shape
    ops = ops or R._Plain()

    def ln(name, t):
        return F.layer_norm(t, (R.D_MODEL,), w[p + name + ".weight"], w[p + name + ".bias"], 1e-5)

    def ffn(name, t):
        t = ops.linear(w, p + name + ".linear1.weight", t, p + name + ".linear1.bias")
        t = t * torch.sigmoid(t)
        return ops.linear(w, p + name + ".linear2.weight", t, p + name + ".linear2.bias")

    r = x
    r = r + 0.5 * ffn("feed_forward1", ln("norm_feed_forward1", r))
    y = ln("norm_self_att", r)
    a = p + "self_attn."
    q = _h(ops.linear(w, a + "linear_q.weight", y, a + "linear_q.bias")).view(B, T, R.N_HEADS, R.D_K)
    k = _h(ops.linear(w, a + "linear_k.weight", y, a + "linear_k.bias")).view(B, T, R.N_HEADS, R.D_K).transpose(1, 2)
    v = _h(ops.linear(w, a + "linear_v.weight", y, a + "linear_v.bias")).view(B, T, R.N_HEADS, R.D_K).transpose(1, 2)
    pp = _h(ops.linear(w, a + "linear_pos.weight", pos_emb, None)).view(1, -1, R.N_HEADS, R.D_K).transpose(1, 2)
    qu = _h(q + w[a + "pos_bias_u"]).transpose(1, 2)
    qv = _h(q + w[a + "pos_bias_v"]).transpose(1, 2)
    bd = R.rel_shift(torch.matmul(qv, pp.transpose(-2, -1)))
    ac = torch.matmul(qu, k.transpose(-2, -1))
    bd = bd[:, :, :, : ac.size(-1)]
    scores = (ac + bd) / math.sqrt(R.D_K)
    valid = ~pad
    att_mask = ~(valid[:, None, :] & valid[:, :, None])
    scores = scores.masked_fill(att_mask[:, None], -10000.0)
    e = torch.exp(scores - scores.max(-1, keepdim=True).values).masked_fill(att_mask[:, None], 0.0)
    ctx = (torch.matmul(_h(e), v) / e.sum(-1, keepdim=True).clamp_min(1e-30)).transpose(1, 2).reshape(B, T, R.D_MODEL)
    r = r + ops.linear(w, a + "linear_out.weight", ctx, a + "linear_out.bias")
    y = ln("norm_conv", r).transpose(1, 2)
    c = p + "conv."
    y = ops.conv(w, c + "pointwise_conv1.weight", y, c + "pointwise_conv1.bias", F.conv1d)
    y = F.glu(y, dim=1).masked_fill(pad[:, None, :], 0.0)
    y = ops.conv(w, c + "depthwise_conv.weight", y, c + "depthwise_conv.bias", F.conv1d, padding=(R.CONV_K - 1) // 2, groups=R.D_MODEL)
    y = F.batch_norm(y, w[c + "batch_norm.running_mean"], w[c + "batch_norm.running_var"], w[c + "batch_norm.weight"],
                     w[c + "batch_norm.bias"], False, 0.0, 1e-5)
    y = y * torch.sigmoid(y)
    r = r + ops.conv(w, c + "pointwise_conv2.weight", y, c + "pointwise_conv2.bias", F.conv1d).transpose(1, 2)
    r = r + 0.5 * ffn("feed_forward2", ln("norm_feed_forward2", r))
    return ln("norm_out", r)


@contextlib.contextmanager
def attention_roundings():
    """with attention_roundings(): R.forward(..., ort=F16Ops()) -- the twin extended by the attention kernels' own roundings"""
    orig = R.conformer_layer
    R.conformer_layer = _layer_with_attention_roundings
    try:
        yield
    finally:
        R.conformer_layer = orig


def _convert_weights():
    name = "convert_weights"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, str(ROOT / "tools" / "convert_weights.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def write_weights(path, w: dict):
    """a NeMo-keyed float32 weight dict as the engine's weight file (tools/convert_weights.py::write_qvw, file order)"""
    C = _convert_weights()
    shapes = C.weight_shapes(C._lib())
    C.write_qvw(path, {k: w[k].numpy() for k in shapes})
    return path


def maxdiff(a, b, n, first: int = 0) -> float:
    """max |a - b| over frames first .. n-1 of one utterance"""
    return float((a[first:n].float().cpu() - b[first:n].float().cpu()).abs().max())


def twin_floor(lp_twin, lp_ref, T) -> list:
    """e per utterance: max |twin - fp32 oracle| over its valid frames"""
    return [maxdiff(lp_twin[b], lp_ref[b], n) for b, n in enumerate(T)]


def decided_frames(lp_ref, e: float):
    """[T] bool: frames whose fp32 top-1 / top-2 log-prob gap exceeds 4 e (an error of e per value cannot swap them)"""
    top = lp_ref.topk(2, -1).values
    return (top[:, 0] - top[:, 1]) > 4.0 * e


def long_lens() -> list:
    """sample counts of the LONG batch: the 766-frame clip is the capacity itself, the others the smallest of their frame count"""
    return [MAX_SAMPLES if t == 766 else samples_for_frames(t) for t in LONG]


def bound_a(e: float) -> float:
    return max(1e-2, FLOOR_K * e)


class _Keep(dict):
    """a taps dict that stores the named activations only (R.forward offers ~70 tensors of [B,T,512])"""

    def __init__(self, names):
        super().__init__()
        self._names = set(names)

    def __setitem__(self, k, v):
        if k in self._names:
            super().__setitem__(k, v)


def reference(w, audio, lens, taps=None, twin: bool = True) -> dict:
    """fp32 oracle (one padded call) and, with `twin`, the f16-operand twin of one batch.  taps: names of the oracle
    activations to keep ('sub', 'layer0', ...).
    {"lp", "t", "taps", "twin", "e" (per utterance), "bound" (rule (a), per utterance)}"""
    tp = _Keep(taps) if taps else None
    lp, t = R.forward(w, audio, lens, taps=tp)
    out = {"lp": lp, "t": t.tolist(), "taps": tp}
    if twin:
        tw, tt = R.forward(w, audio, lens, ort=F16Ops())
        assert tt.tolist() == out["t"]
        out["twin"] = tw
        with attention_roundings():
            out["twin_att"] = R.forward(w, audio, lens, ort=F16Ops())[0]
        out["e"] = twin_floor(tw, lp, out["t"])
        out["bound"] = [bound_a(e) for e in out["e"]]
    return out


def planted(w, audio, lens, rows) -> dict:
    """the fp32 oracle under each planted error on the utterances `rows` of a batch (the oracle is batch-invariant to
    1e-5, test_forward_ref_host.py): {"positions": {row: lp [T,1025]}, "last_frame": {...}}"""
    rows = list(rows)
    sub_lens = [lens[r] for r in rows]
    sub = audio[rows][:, : max(sub_lens)].contiguous()
    out = {}
    for key, cm in (("positions", positions_off_by_one), ("last_frame", last_frame_dropped)):
        with cm():
            lp, t = R.forward(w, sub, sub_lens)
        out[key] = {r: lp[i, : int(t[i])] for i, r in enumerate(rows)}
    return out


def check_rules(tag, got, ref, rows=None) -> list:
    """rule (a) per utterance, asserted; the distance of rule (b) and the one from the twin with the attention kernels'
    roundings are printed only (see the module docstring).  got = device log-probs [B,T,1025]."""
    T = ref["t"]
    figures = []
    for b in (range(len(T)) if rows is None else rows):
        n = T[b]
        da = maxdiff(got[b], ref["lp"][b], n)
        db = maxdiff(got[b], ref["twin"][b], n)
        figures.append((n, ref["e"][b], da, db))
        print(f"[fwd-len] {tag} T={n}: e {ref['e'][b]:.3e}  (a) device vs fp32 {da:.3e} <= {ref['bound'][b]:.3e}  "
              f"(b) device vs twin {db:.3e} = {db / ref['e'][b]:.2f} e   [twin + attention roundings: vs fp32 "
              f"{maxdiff(ref['twin_att'][b], ref['lp'][b], n):.3e}, device vs it {maxdiff(got[b], ref['twin_att'][b], n):.3e}]")
    for (n, e, da, db), b in zip(figures, (range(len(T)) if rows is None else rows)):
        assert da <= ref["bound"][b], (tag, n, "rule (a)", da, ref["bound"][b])
    return figures
