"""Reference-side helpers for the length tests and the per-layer tap tests of the acoustic forward
(tests/test_gpu_forward_lengths.py, tests/test_gpu_layer_taps.py, tests/test_gpu_ort_layers.py, tests/test_forward_ref_host.py).  Everything here runs on the CPU with oracle/fastconformer_ref.py alone.

  * the twin (`F16Ops`): the fp32 restatement with the ONE rounding the device design chooses -- float16 operands of every
    Linear / Conv, float32 accumulation and bias.  Its distance `e` from the fp32 restatement is the reference-side floor
    the device is judged against: (a) device vs fp32 <= max(1e-2, FLOOR_K * e).  The device's distance from the twin --
    rule (b), "<= e" -- is printed and NOT asserted: measured, it is 0.58 - 1.04 e (0.6 - 1.13 e from the twin with the
    attention kernels' roundings), i.e. two f16-operand evaluations lie about as far from each other as from fp32.
  * `sharp_weights`: the seeded random weights with the attention's query side x4, on which the relative-position term
    is visible in the log-probs while `e` does not move.
  * two PLANTED reference errors (context managers): what a position off-by-one or a dropped last key frame in an
    attention kernel would compute.  A test whose bound such an oracle passes proves nothing about that error.
  * `telltale_weights`, `PLANTS`, `layer_power`, `tap_floor` (second half of the file): the weight set on which one wrong
    tensor in one layer shows at the tap behind that layer, the 46 wrong tensors, what each does to each of the 17 taps,
    and the taps' own float16 floor.
  * `ort_layer`, `OrtOps`, `ort_twins`, `ort_segments`, `telltale_ort_weights`, `PLANTS2` (last part of the file): precision 2 --
    one layer of the OrtMixed oracle with the conv module cut out, the twins whose envelope bounds the device there, and the
    precision-2 plants (tests/test_gpu_ort_layers.py).
  * `POISON_KINDS`, `poisoned`: the non-finite rows (and the harmless "loud" one) of tests/test_gpu_forward_isolation.py and
    tests/test_forward_isolation_host.py.
"""

from __future__ import annotations

import contextlib
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
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


# Rows that must not reach their neighbours or the next batch (tests/test_forward_isolation_host.py shows on the oracle that
# each POISON kind really leaves no finite log-prob in its own row, and that "loud" is harmless):
#   nan       every sample NaN
#   pos_inf   one +inf sample in the middle of an otherwise normal clip
#   neg_inf   one -inf sample there
#   huge      the clip times 1e30: finite samples whose power spectrum overflows float32
#   nan_tail  NaN in the last 400 samples only
POISON_KINDS = ("nan", "pos_inf", "neg_inf", "huge", "nan_tail")
LOUD_GAIN = 32768.0      # "loud": a normal clip in unscaled int16 units -- finite everywhere


def poisoned(clip: torch.Tensor, n: int, kind: str) -> torch.Tensor:
    """a copy of the 1-D `clip` (n samples, zeros behind them) made into poison row `kind`, or "loud"; still zero behind n"""
    out = clip.clone()
    if kind == "nan":
        out[:n] = float("nan")
    elif kind == "pos_inf":
        out[n // 2] = float("inf")
    elif kind == "neg_inf":
        out[n // 2] = float("-inf")
    elif kind == "huge":
        out[:n] *= 1e30
    elif kind == "nan_tail":
        out[max(0, n - 400): n] = float("nan")
    elif kind == "loud":
        out[:n] *= LOUD_GAIN
    else:
        raise KeyError(kind)
    return out


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
    (csrc/qv_attention.hip: k_attention*): q, k, v and the projected position rows are STORED as float16, q + u and q + v are
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


# ------------------------------------------------------------------ every layer, every tensor ---------------------------
# tests/test_gpu_layer_taps.py holds the tap behind each of the 17 layers to the fp32 oracle; what follows is the reference
# side of it: a weight set on which ONE wrong per-layer tensor shows at that layer's tap, the wrong tensors themselves
# ("plants": the oracle evaluated on misrouted weights, never a kernel), and the precision floor of the taps.

TAP_BOUND = 1.5e-2            # the project's bound on a layer tap (test_gpu_forward.py, test_gpu_forward_lengths.py)
SUB_BOUND = 5e-2              # ... and on the sqrt(512)-scaled subsampling output
_L0 = "encoder.layers.0."
LAYER_SUFFIXES = tuple(k[len(_L0):] for k in R.weight_shapes(1) if k.startswith(_L0))       # the 39 tensors of a layer
UNOBSERVABLE = "self_attn.linear_k.bias"

# gains on top of sharp_weights(); "running_var" is spread around 1, not scaled.  See telltale_weights().
TELLTALE_OUT_GAIN = 1.0 / 16.0
TELLTALE_VAR_SPREAD = 6.0
TELLTALE_GAINS = (("self_attn.pos_bias_u", 16.0), ("self_attn.pos_bias_v", 5.0), ("self_attn.linear_q.bias", 6.0),
                  ("conv.batch_norm.running_mean", 5.0))


def telltale_weights(w: dict) -> dict:
    """The weight set on which a wrong tensor in ANY layer moves that layer's tap by >= 4x the tap bound
    (test_forward_ref_host.py::test_every_plant_shows_at_its_layer_tap).  sharp_weights(w), and then:

      * pre_encode.out weight and bias x 1/16: the encoder's input stream is sub * sqrt(512), +-30 on the seeded weights, so
        in layer 0 every branch output (O(1)) is a 3 % ripple that norm_out shrinks to the size of the tap bound.  With 1/16
        the stream entering layer 0 is O(1) like the one entering layers 1 .. 16 (each a norm_out output).
      * batch_norm.running_var = 1 + 6 (v - 1): the seeded variances lie in 1 .. 1.3, so a neighbour's differs by a few
        per cent, in a tensor that a Swish and a pointwise conv still follow.  Spread to 1 .. 2.8 it changes the scale by
        tens of per cent (and stays positive: v >= 1).
      * batch_norm.running_mean x5: "mean not scaled by gamma / sqrt(var + eps)" is an error of mean * (1 - 1 / s); with
        the seeded mean (std 0.1) and s within 0.6 .. 1.1 that is 1.3 bounds in the worst layer, x5 makes it >= 6.
      * pos_bias_u x16, pos_bias_v x5, linear_q.bias x6 (on top of the sharp x4): the three vectors that reach the output
        only through a product with a key / position row inside the softmax.  At the sharp gain a neighbour's vector moves
        a tap by 3e-2 - 5e-2 in the best layer and 6e-3 in the worst.  u needs most: u.k is the same for every query of a
        head and only re-weights the keys, where v.p also moves the position profile.

    What was tried and left out: linear_k.weight x1.5 (with u x12, v x4, q.bias x4) reaches the same power, but the sharper
    softmax doubles the taps' own float16 floor (e_tap 1.1e-2 in layers 2 - 5: 1.5 e_tap would then BE the bound).  With
    the keys left alone e_tap stays <= 8.1e-3.  Gains on the additive biases (every Linear / conv bias x4 or x8) do not work
    either: the late layers saturate (Swish, softmax) and the early layers' deviations are normalised away by the norm_out's
    that follow before they reach the log-probs (0.0 - 0.5 bounds there); the taps do not need them -- with O(1) layer
    inputs a neighbour's bias (std 0.1) is already > 5 bounds.

    linear_k.bias stays invisible on any weights: test_key_bias_is_invisible_by_construction."""
    out = sharp_weights(w)
    for name in ("encoder.pre_encode.out.weight", "encoder.pre_encode.out.bias"):
        out[name] = (out[name] * TELLTALE_OUT_GAIN).contiguous()
    for name in list(out):
        if not name.startswith("encoder.layers."):
            continue
        if name.endswith("conv.batch_norm.running_var"):
            out[name] = (1.0 + TELLTALE_VAR_SPREAD * (out[name] - 1.0)).contiguous()
        for suffix, gain in TELLTALE_GAINS:
            if name.endswith(suffix):
                out[name] = (out[name] * gain).contiguous()
    return out


def _p(l: int) -> str:
    return f"encoder.layers.{l}."


def _misroute(suffix):
    def plant(w, l):
        return {_p(l) + suffix: w[_p((l + 1) % R.N_LAYERS) + suffix]}
    return plant


def _swap(a, b):
    def plant(w, l):
        return {_p(l) + a: w[_p(l) + b], _p(l) + b: w[_p(l) + a]}
    return plant


def _swap_norms(w, l):
    out = {}
    for part in (".weight", ".bias"):
        out.update(_swap("norm_feed_forward1" + part, "norm_feed_forward2" + part)(w, l))
    return out


def _depthwise(change):
    def plant(w, l):
        name = _p(l) + "conv.depthwise_conv.weight"
        return {name: change(w[name].clone()).contiguous()}
    return plant


def _drop_tap(k):
    def change(t):
        t[..., k] = 0.0
        return t
    return change


def _mean_not_scaled(w, l):
    """BatchNorm folded to y = x * s + (beta - mean * s), s = gamma / sqrt(var + eps), with the `* s` on the mean forgotten:
    y = x * s + beta - mean.  The same thing as a running_mean of mean / s."""
    c = _p(l) + "conv.batch_norm."
    s = w[c + "weight"] / torch.sqrt(w[c + "running_var"] + 1e-5)
    return {c + "running_mean": (w[c + "running_mean"] / s).contiguous()}


# name -> plant(w, l): the entries of the weight dict that layer l reads wrongly
MISROUTES = {"next:" + s: _misroute(s) for s in LAYER_SUFFIXES}
STRUCTURAL = {
    "swap:pos_bias_u<->pos_bias_v": _swap("self_attn.pos_bias_u", "self_attn.pos_bias_v"),
    "swap:norm_feed_forward1<->norm_feed_forward2": _swap_norms,
    "swap:feed_forward1<->feed_forward2.linear2.bias": _swap("feed_forward1.linear2.bias", "feed_forward2.linear2.bias"),
    "depthwise:taps reversed": _depthwise(lambda t: t.flip(-1)),
    "depthwise:first tap dropped": _depthwise(_drop_tap(0)),
    "depthwise:last tap dropped": _depthwise(_drop_tap(R.CONV_K - 1)),
    "batch_norm:mean not scaled": _mean_not_scaled,
}
PLANTS = {**MISROUTES, **STRUCTURAL}
BLIND = "next:" + UNOBSERVABLE                 # the one plant no output can see
LAYER_TAPS = ["sub"] + [f"layer{l}" for l in range(R.N_LAYERS)]


def _rows_of(audio, lens, rows):
    rows = list(rows)
    sub_lens = [lens[r] for r in rows]
    return audio[rows][:, : max(sub_lens)].contiguous(), sub_lens


def _tap_dist(a, b, T) -> float:
    """max |a - b| over the valid frames of every utterance"""
    return max(maxdiff(a[i], b[i], n) for i, n in enumerate(T))


@torch.no_grad()
def layer_power(w, audio, lens, rows, against=None, plants=None, layers=None) -> dict:
    """What each plant does to each layer's tap, on the utterances `rows` of a batch.  The fp32 oracle runs once with `sub`
    and all 17 layer taps kept; a plant in layer l is then ONE R.conformer_layer call on the oracle's own input to layer l
    (a wrong tensor of layer l cannot reach tap l any other way), so the 46 x 17 table costs about as much as 46 forwards
    of two short clips.
    `layers`: the layers to plant in (default: all 17; the lists below then have one entry per layer given).
    {"t", "taps", "D": {plant: [17 distances planted vs true tap]}, "reeval": [17 distances of the unplanted re-evaluation
     from the oracle's tap -- 0.0 each, test_single_layer_reevaluation_is_the_oracle], and with against = {l: tensor
     [len(rows), >= T, 512]} (a device's taps of those rows) "A": {plant: [17 distances planted vs `against`]}}"""
    sub_audio, sub_lens = _rows_of(audio, lens, rows)
    taps = _Keep(LAYER_TAPS)
    _, t = R.forward(w, sub_audio, sub_lens, taps=taps)
    T = t.tolist()
    tmax = taps["sub"].shape[1]
    pos_emb = R.rel_pos_emb(tmax).unsqueeze(0)
    pad = torch.arange(tmax)[None, :] >= t[:, None]
    plants = PLANTS if plants is None else plants
    out = {"t": T, "taps": taps, "D": {k: [] for k in plants}, "reeval": []}
    if against is not None:
        out["A"] = {k: [] for k in plants}
    for l in (range(R.N_LAYERS) if layers is None else layers):
        x = taps["sub"] * math.sqrt(R.D_MODEL) if l == 0 else taps[f"layer{l - 1}"]
        true = taps[f"layer{l}"]
        out["reeval"].append(_tap_dist(R.conformer_layer(w, _p(l), x, pos_emb, pad), true, T))
        for key, plant in plants.items():
            bad = R.conformer_layer({**w, **plant(w, l)}, _p(l), x, pos_emb, pad)
            out["D"][key].append(_tap_dist(bad, true, T))
            if against is not None:
                out["A"][key].append(_tap_dist(bad, against[l][:, :tmax], T))
    return out


@torch.no_grad()
def tap_floor(w, audio, lens, taps=None) -> dict:
    """e_tap per layer: the larger of the two reference twins' distances (F16Ops; F16Ops with the attention kernels' roundings)
    from the fp32 oracle's tap, over the valid frames of every utterance; `taps` = the fp32 oracle's, if already at hand.
    {"t", "taps" (fp32), "lp", "twin", "twin_att", "e", "bound" (rule (a), per utterance), "e_tap" [17], "bound_tap" [17],
     "e_sub"}"""
    if taps is None:
        taps = _Keep(LAYER_TAPS)
        lp, t = R.forward(w, audio, lens, taps=taps)
    else:
        lp, t = R.forward(w, audio, lens)
    T = t.tolist()
    tw_taps, att_taps = _Keep(LAYER_TAPS), _Keep(LAYER_TAPS)
    tw, _ = R.forward(w, audio, lens, taps=tw_taps, ort=F16Ops())
    with attention_roundings():
        tw_att, _ = R.forward(w, audio, lens, taps=att_taps, ort=F16Ops())
    e_tap = [max(_tap_dist(tw_taps[k], taps[k], T), _tap_dist(att_taps[k], taps[k], T)) for k in LAYER_TAPS[1:]]
    e = twin_floor(tw, lp, T)
    return {"t": T, "taps": taps, "lp": lp, "twin": tw, "twin_att": tw_att, "e": e, "bound": [bound_a(x) for x in e],
            "e_tap": e_tap, "bound_tap": [bound_tap(x) for x in e_tap],
            "e_sub": math.sqrt(R.D_MODEL) * max(_tap_dist(tw_taps["sub"], taps["sub"], T), _tap_dist(att_taps["sub"], taps["sub"], T))}


def bound_tap(e: float) -> float:
    return max(TAP_BOUND, FLOOR_K * e)


# ------------------------------------------------------------------ precision 2: every layer, quantisers cut out -------
# tests/test_gpu_ort_layers.py holds every layer of a QV_PREC_ORT_MIXED engine to the OrtMixed oracle; what follows is the
# reference side of it.  A whole layer cannot be compared tightly: the three DynamicQuantizeLinear sites of the conv module
# are rounding discontinuities, and two evaluations that differ by a float16 rounding flip a few activations across them
# (0.8e-2 - 2.3e-2 at the layer output, measured oracle against oracle).  So the layer is cut where the device exposes its
# tensors:  segment A  layer input -> norm_conv's output `lnc` (no quantiser in it);  the exact stages lnc -> GLU -> `dw`
# (integer arithmetic, 1e-5 of range);  segment C  layer input AND the depthwise stage's output `dw` -> layer output, in which
# pointwise_conv2 quantises the SAME tensor on both sides and nothing flips.

ORT_CONVS = ("conv.pointwise_conv1.weight", "conv.depthwise_conv.weight", "conv.pointwise_conv2.weight")
ORT_CONV_GAINS = (1.0, 1.5, 2.25)     # layer l: every ORT_CONVS weight x ORT_CONV_GAINS[l % 3].  See telltale_ort_weights().
STAGE_REL = 1e-5                      # an exact stage: max |d| <= 1e-5 of the expected tensor's range (test_gpu_ort_mixed.py::_report)
SUB_OUT = "encoder.pre_encode.out.weight"


def telltale_ort_weights(w: dict) -> dict:
    """telltale_weights(w), and each layer's three conv weights (pointwise_conv1, depthwise_conv, pointwise_conv2) times
    ORT_CONV_GAINS[l % 3] = 1 / 1.5 / 2.25.  Biases are untouched.

    Why: a precision-2 engine holds ONE int8 scale per conv tensor, max|w| / 127.  On the seeded weights the maxima of
    neighbouring layers differ by 1 - 2 %, so a launch that rescales the right integers with the neighbour's scale moves the
    layer output by 0.008 - 0.023 -- a few twin distances only.  With the gains a neighbour's scale (layer (l + 1) % 17; 16 -> 0
    is 1.5 against 1) is 1.5x larger or 2.25x smaller, never within a third.

    How the gains were chosen (33- and 129-frame clips, 17 layers; test_forward_ref_host.py prints the tables):
      * no gain below 1: a zero point off by one is an error of s_x s_w sum(w_q) per output channel, proportional to the
        gain.  It is the weakest plant: in the layers whose gain is 1, pointwise_conv2's lies 5.9 - 18 bounds from the oracle
        at the layer output (4 are asked); a gain of 0.7 would take the weakest of them to about 4.
      * 1 / 1.5 / 2.25, the only set measured in full: the twins' envelopes are 1.4e-3 - 4.7e-3 at `lnc` and 0.5e-3 - 4.7e-3 at
        the layer output (largest bound 7.1e-3, below TAP_BOUND), every plant in front of `lnc` lies >= 40 bounds away there,
        every plant outside the cut-out chain >= 5.9 bounds at the layer output (the next weakest after the zero point: 17),
        and every plant inside the chain moves its stage tensor by >= 970 stage bounds.  Larger gains were not needed and not
        tried: they would let the conv branch outweigh the residual stream that the feed_forward2 plants are measured on."""
    out = telltale_weights(w)
    for l in range(R.N_LAYERS):
        for suffix in ORT_CONVS:
            out[_p(l) + suffix] = (out[_p(l) + suffix] * ORT_CONV_GAINS[l % 3]).contiguous()
    return out


_INT4_CACHE = {}          # (mode, id(tensor)) -> (tensor, dequantised); the newest _INT4_KEEP entries (two layers' worth and more)
_INT4_KEEP = 64


def _int4_values(wt, mode):
    key = (mode, id(wt))
    hit = _INT4_CACHE.get(key)
    if hit is None or hit[0] is not wt:
        fn = R.quant_dequant_int4_f32scale if mode == "f32scale" else R.quant_dequant_int4
        hit = (wt, torch.from_numpy(fn(wt.numpy())))
        _INT4_CACHE[key] = hit
        while len(_INT4_CACHE) > _INT4_KEEP:
            _INT4_CACHE.pop(next(iter(_INT4_CACHE)))
    return hit[1]


class OrtOps(R.OrtMixed):
    """R.OrtMixed (bit for bit, test_ort_ops_without_options_are_the_oracle) with
      * prepared weights looked up by TENSOR, not by name, so that a weight dict with one entry misrouted can be evaluated
        with the same object (OrtMixed caches by name);
      * the perturbations the precision-2 twins are made of:
          f16_inputs   every Linear input rounded to float16 -- ort_floor.make_f16_input_ops's rounding;
          int4         "f32scale": the oracle's (q - 8) * scale, scale in float32;
                       "f16scale": the block scale kept in float16 (R.quant_dequant_int4; fastconformer_ref.py:270-271);
                       "device":   the operand the W4A16 GEMM multiplies by, half((q - 8) * half(scale)): dequant8 rounds the
                                   product once to float16 (csrc/qv_gemm_dequant.h:17).  pre_encode.out is the exception: it is
                                   dequantised with the float32 scale on the host and stored as float16,
                                   half((q - 8) * scale) (csrc/qv_model_prep_host.h:291-296);
          noise        (eps, seed): relative noise on every Linear input -- ort_floor.make_noise_ops's;
      * `plant` = {conv weight name: (kind, neighbour's weight name)}: what a launch of that conv with a wrong quantisation
        parameter computes, the integers right --
          "scale"   the int32 sums rescaled with the NEIGHBOUR tensor's int8 scale;
          "zp+1"    the activation zero point off by one (255 -> 254);
          "nozp"    the zero-point correction dropped: sum(x_q w_q) instead of sum((x_q - zp) w_q)."""

    def __init__(self, f16_inputs: bool = False, int4: str = "f32scale", noise=None, plant=None):
        super().__init__()
        assert int4 in ("f32scale", "f16scale", "device")
        self.f16_inputs, self.int4, self.plant = f16_inputs, int4, dict(plant or {})
        self.eps, self.g = (noise[0], torch.Generator().manual_seed(noise[1])) if noise else (0.0, None)

    def _linear_weight(self, wt, name):
        if name == SUB_OUT:
            v = _int4_values(wt, "f32scale")
            return v.half().float() if self.int4 == "device" else v
        if not name.endswith(R.INT4_LINEAR_SUFFIXES):
            return wt
        if self.int4 == "f32scale":
            return _int4_values(wt, "f32scale")
        v = _int4_values(wt, "f16scale")
        return v.half().float() if self.int4 == "device" else v

    def linear(self, w, name, x, bias_name):
        if self.g is not None:
            x = x * (1 + self.eps * (torch.rand(x.shape, generator=self.g) * 2 - 1))
        if self.f16_inputs:
            x = x.half().float()
        return F.linear(x, self._linear_weight(w[name], name), w[bias_name] if bias_name else None)

    def _int8(self, wt):
        hit = self._w8.get(id(wt))
        if hit is None or hit[0] is not wt:
            hit = (wt, R.quantize_weight_int8(wt))
            self._w8[id(wt)] = hit
        return hit[1]

    def conv(self, w, name, x, bias_name, fn, **kw):
        bias = w[bias_name] if bias_name else None
        wq, sw = self._int8(w[name])
        kind, other = self.plant.get(name, (None, None))
        if kind == "scale":
            sw = self._int8(w[other])[1]
        outs = []
        for b in range(x.shape[0]):
            xq, sx, zp = R.dynamic_quantize_linear(x[b: b + 1])
            if kind == "zp+1":
                zp = zp + 1.0 if zp < 255.0 else zp - 1.0
            elif kind == "nozp":
                zp = 0.0
            acc = fn(xq - zp, wq, None, **kw)
            y = (acc * float(np.float32(sx) * np.float32(sw))).to(torch.float32)
            outs.append(y + bias.view(1, -1, *([1] * (y.dim() - 2))) if bias is not None else y)
        return torch.cat(outs, 0)


ORT_PLANTS = {f"ort:{s.split('.')[1]}:{what}": (s, kind) for s in ORT_CONVS
              for what, kind in (("neighbour's int8 scale", "scale"), ("zero point off by one", "zp+1"), ("zero-point correction dropped", "nozp"))}
PLANTS2 = {**PLANTS, **{k: None for k in ORT_PLANTS}}          # the 46 + 9 plants of precision 2, by name
# the plants inside the chain the cut removes (pointwise_conv1 -> GLU -> depthwise_conv -> BatchNorm -> Swish): with `dw`
# handed over they cannot reach the layer output; the exact stage behind them owns them ("glu": lnc -> GLU, "dw": GLU -> dw)
_CHAIN = {"conv.pointwise_conv1.": "glu", "conv.depthwise_conv.": "dw", "conv.batch_norm.": "dw", "depthwise:": "dw",
          "batch_norm:": "dw", "ort:pointwise_conv1:": "glu", "ort:depthwise_conv:": "dw"}
# ... and the tensors in front of norm_conv's output: a plant there shows at `lnc` already
_FRONT = ("norm_feed_forward1.", "feed_forward1.", "norm_self_att.", "self_attn.", "norm_conv.", "swap:")


def plant_stage(key: str):
    """'glu' / 'dw' for a plant inside the cut-out chain (the stage tensor that shows it), None otherwise"""
    body = key[len("next:"):] if key.startswith("next:") else key
    return next((stage for prefix, stage in _CHAIN.items() if body.startswith(prefix)), None)


def plant_shows_at_lnc(key: str) -> bool:
    body = key[len("next:"):] if key.startswith("next:") else key
    return key != BLIND and body.startswith(_FRONT)


def plant_shows_at_out(key: str) -> bool:
    """every observable plant outside the cut-out chain -- but norm_conv's weight and bias: norm_conv's output feeds the chain and
    nothing else, so with `dw` handed over they cannot reach the layer output either.  `lnc` is their tensor (segment A)."""
    body = key[len("next:"):] if key.startswith("next:") else key
    return key != BLIND and plant_stage(key) is None and not body.startswith("norm_conv.")


def planted2(key: str, w: dict, l: int):
    """(weights, ops) with plant `key` in layer l, for the OrtMixed oracle"""
    if key in ORT_PLANTS:
        suffix, kind = ORT_PLANTS[key]
        return w, OrtOps(plant={_p(l) + suffix: (kind, _p((l + 1) % R.N_LAYERS) + suffix)})
    return {**w, **PLANTS[key](w, l)}, OrtOps()


def ort_layer(w, p, x, ops, dw=None, att16: bool = False) -> dict:
    """R.conformer_layer restated for ONE unpadded utterance x [1, T, 512] (no padding mask anywhere), with the conv module cut
    open: returns {"lnc": norm_conv's output, "dw": the depthwise stage's output, "out": the layer's output}, each [1, T, 512],
    and with `dw` given that tensor takes the place of pointwise_conv1 -> GLU -> depthwise_conv -> BatchNorm -> Swish.
    Under OrtMixed it gives R.conformer_layer's bits, with nothing given and with its own `dw` given back
    (test_forward_ref_host.py::test_cut_layer_restates_the_oracle_layer).  att16: the attention as
    _layer_with_attention_roundings computes it (the attention kernels' float16 roundings)."""
    assert x.dim() == 3 and x.shape[0] == 1
    T = x.shape[1]

    def ln(name, t):
        return F.layer_norm(t, (R.D_MODEL,), w[p + name + ".weight"], w[p + name + ".bias"], 1e-5)

    def ffn(name, t):
        t = ops.linear(w, p + name + ".linear1.weight", t, p + name + ".linear1.bias")
        t = t * torch.sigmoid(t)
        return ops.linear(w, p + name + ".linear2.weight", t, p + name + ".linear2.bias")

    h = _h if att16 else (lambda t: t)
    r = x
    r = r + 0.5 * ffn("feed_forward1", ln("norm_feed_forward1", r))
    y = ln("norm_self_att", r)
    a = p + "self_attn."
    q = h(ops.linear(w, a + "linear_q.weight", y, a + "linear_q.bias")).view(1, T, R.N_HEADS, R.D_K)
    k = h(ops.linear(w, a + "linear_k.weight", y, a + "linear_k.bias")).view(1, T, R.N_HEADS, R.D_K).transpose(1, 2)
    v = h(ops.linear(w, a + "linear_v.weight", y, a + "linear_v.bias")).view(1, T, R.N_HEADS, R.D_K).transpose(1, 2)
    pp = h(ops.linear(w, a + "linear_pos.weight", R.rel_pos_emb(T).unsqueeze(0), None)).view(1, -1, R.N_HEADS, R.D_K).transpose(1, 2)
    qu = h(q + w[a + "pos_bias_u"]).transpose(1, 2)
    qv = h(q + w[a + "pos_bias_v"]).transpose(1, 2)
    bd = R.rel_shift(torch.matmul(qv, pp.transpose(-2, -1)))
    ac = torch.matmul(qu, k.transpose(-2, -1))
    bd = bd[:, :, :, : ac.size(-1)]
    scores = (ac + bd) / math.sqrt(R.D_K)
    if att16:
        e = torch.exp(scores - scores.max(-1, keepdim=True).values)
        ctx = torch.matmul(_h(e), v) / e.sum(-1, keepdim=True).clamp_min(1e-30)
    else:
        ctx = torch.matmul(torch.softmax(scores, dim=-1), v)
    ctx = ctx.transpose(1, 2).reshape(1, T, R.D_MODEL)
    r = r + ops.linear(w, a + "linear_out.weight", ctx, a + "linear_out.bias")
    y = ln("norm_conv", r).transpose(1, 2)
    out = {"lnc": y.transpose(1, 2).contiguous()}
    c = p + "conv."
    if dw is None:
        out["glu"] = ort_stage(w, p, "glu", out["lnc"][0], ops).unsqueeze(0)
        out["dw"] = ort_stage(w, p, "dw", out["glu"][0], ops).unsqueeze(0)
        dw = out["dw"]
    else:
        out["dw"] = dw
    y = ops.conv(w, c + "pointwise_conv2.weight", dw.transpose(1, 2), c + "pointwise_conv2.bias", F.conv1d).transpose(1, 2)
    r = r + y
    r = r + 0.5 * ffn("feed_forward2", ln("norm_feed_forward2", r))
    out["out"] = ln("norm_out", r)
    return out


def ort_stage(w, p, stage: str, x, ops):
    """one exact stage of layer `p`'s conv module on x [T, 512] -> [T, 512], as R.conformer_layer computes it for an unpadded
    utterance: "glu" = pointwise_conv1 + GLU of norm_conv's output, "dw" = depthwise_conv + BatchNorm + Swish of GLU's output"""
    c = p + "conv."
    y = x.t().unsqueeze(0)
    if stage == "glu":
        y = F.glu(ops.conv(w, c + "pointwise_conv1.weight", y, c + "pointwise_conv1.bias", F.conv1d), dim=1)
    else:
        y = ops.conv(w, c + "depthwise_conv.weight", y, c + "depthwise_conv.bias", F.conv1d, padding=(R.CONV_K - 1) // 2, groups=R.D_MODEL)
        y = F.batch_norm(y, w[c + "batch_norm.running_mean"], w[c + "batch_norm.running_var"], w[c + "batch_norm.weight"],
                         w[c + "batch_norm.bias"], False, 0.0, 1e-5)
        y = y * torch.sigmoid(y)
    return y[0].t().contiguous()


def ort_pre_encode(w, c2p, ops):
    """pre_encode.out and the xscaling on the channels-last conv.6 output c2p [T, 10, 256] of one utterance -> [T, 512]: the
    encoder's input as R.subsampling + R.forward compute it (NeMo flattens [C][F] as c * 10 + f)"""
    x = c2p.permute(0, 2, 1).reshape(1, c2p.shape[0], R.SUB_CH * 10)
    return ops.linear(w, SUB_OUT, x, "encoder.pre_encode.out.bias")[0] * math.sqrt(R.D_MODEL)


def ort_twins() -> dict:
    """name -> (ops, att16): the evaluations whose envelope around the OrtMixed oracle is `e`.  None of them is an error: each
    is the oracle with roundings a precision-2 engine performs BY DESIGN, or with noise far below any tolerance.
      f16in              Linear inputs rounded to float16: the f16-operand MFMA GEMM's A operand (LayerNorm, Swish and attention
                         outputs are stored as float16: csrc/qv_model.hip ffn_half / attention_block write a.ln, a.hbuf, a.att)
      f16in+f16scale     ... and the int4 block scales kept in float16 (csrc/qv_wpack_host.h::qv_pack_w4)
      device             ... and the dequantised weight rounded once to the float16 B operand (csrc/qv_gemm_dequant.h:17)
      device+attention   ... and the attention kernels' own roundings (attention_roundings(), csrc/qv_attention.hip)
      noise1, noise2     the oracle with 1e-7 relative noise on every Linear input (ort_floor.make_noise_ops)"""
    return {"f16in": (OrtOps(f16_inputs=True), False),
            "f16in+f16scale": (OrtOps(f16_inputs=True, int4="f16scale"), False),
            "device": (OrtOps(f16_inputs=True, int4="device"), False),
            "device+attention": (OrtOps(f16_inputs=True, int4="device"), True),
            "noise1": (OrtOps(noise=(1e-7, 1)), False), "noise2": (OrtOps(noise=(1e-7, 2)), False)}


def _d(a, b) -> float:
    return float((a.float() - b.float()).abs().max())


@torch.no_grad()
def ort_segments(w, l: int, x, dw, twins=None, plants=(), against=None) -> dict:
    """Layer l of the OrtMixed oracle on ONE utterance's layer input x [T, 512] with the depthwise stage's output dw [T, 512]
    handed over.  {"lnc", "out": the oracle's two tensors [T, 512];  "e_lnc", "e_out": the twins' envelope, max over `twins`
    (ort_twins()) of max |twin - oracle|, and "rows": the same per twin;  "D": {plant: (distance at lnc, at out) of the planted
    oracle from the true one};  with against = (lnc, out) of a device, "A": {plant: ...} the planted oracle's distances from
    those}.  The twins get the same x and dw: `e` is measured on the very input the device is judged on."""
    p = _p(l)
    x, dw = x.unsqueeze(0), dw.unsqueeze(0)
    ref = ort_layer(w, p, x, OrtOps(), dw)
    out = {"lnc": ref["lnc"][0], "out": ref["out"][0], "rows": {}, "D": {}, "A": {}}
    for name, (ops, att16) in (twins or {}).items():
        t = ort_layer(w, p, x, ops, dw, att16)
        out["rows"][name] = (_d(t["lnc"], ref["lnc"]), _d(t["out"], ref["out"]))
    if twins:
        out["e_lnc"] = max(r[0] for r in out["rows"].values())
        out["e_out"] = max(r[1] for r in out["rows"].values())
    for key in plants:
        wp, ops = planted2(key, w, l)
        bad = ort_layer(wp, p, x, ops, dw)
        out["D"][key] = (_d(bad["lnc"], ref["lnc"]), _d(bad["out"], ref["out"]))
        if against is not None:
            out["A"][key] = (_d(bad["lnc"][0], against[0]), _d(bad["out"][0], against[1]))
    return out


@torch.no_grad()
def ort_pre_encode_floor(w, c2p) -> dict:
    """{"ref": the oracle's encoder input [T, 512] from c2p [T, 10, 256], "e", "rows"}: the envelope of the twins that touch a
    Linear (ort_twins() without the attention one)"""
    ref = ort_pre_encode(w, c2p, OrtOps())
    rows = {name: _d(ort_pre_encode(w, c2p, ops), ref) for name, (ops, att16) in ort_twins().items() if not att16}
    return {"ref": ref, "rows": rows, "e": max(rows.values())}
