"""The premises of tests/test_gpu_forward_lengths.py, checked with the reference alone (CPU, oracle/fastconformer_ref.py):
the f16-operand twin's distance `e` from the fp32 restatement is below 1e-2 on the "sharp attention" weights and within
2x of what it is on the plain ones, the two planted errors stand out of the bound there (and the position error does
NOT on the plain weights -- the gap those tests close), the structured set's argmax condition leaves (almost) no frame
out, and the oracle is batch-invariant, so one padded call serves a ragged device batch.

Second half, the premises of tests/test_gpu_layer_taps.py: on forward_ref.telltale_weights every per-layer tensor read from the
neighbouring layer, and seven slips inside a layer, move that layer's tap by >= 4 tap bounds in all 17 layers, while the taps' own
float16 floor leaves the bound at the project's 1.5e-2; linear_k.bias alone is invisible, by construction; and on the sharp weights
layer 0 hides such errors."""

import pytest
import torch

import forward_ref as FR
from oracle import fastconformer_ref as R

SEED = 7
FRAMES = [1, 33, 129, 257]          # the ladder's shortest and longest clip and two in between, cut from the ladder's audio
CHECKED = [1, 2, 3]                 # rows of T = 33, 129, 257


@pytest.fixture(scope="module")
def refs():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ladder = [FR.samples_for_frames(t) for t in FR.LADDER]
    rows = [FR.LADDER.index(t) for t in FRAMES]
    lens = [ladder[r] for r in rows]
    audio = FR.clips(ladder, FR.LADDER_AUDIO_SEED)[rows][:, : max(lens)].contiguous()
    plain = R.random_weights(SEED)
    sharp = FR.sharp_weights(plain)
    out = dict(audio=audio, lens=lens, plain_w=plain, sharp_w=sharp,
               sharp=FR.reference(sharp, audio, lens), plain=FR.reference(plain, audio, lens))
    assert out["sharp"]["t"] == FRAMES
    return out


def test_sharp_weights_touch_the_query_side_only(refs):
    changed = [k for k in refs["plain_w"] if not torch.equal(refs["plain_w"][k], refs["sharp_w"][k])]
    assert len(changed) == 4 * R.N_LAYERS and all(k.endswith(FR.SHARP_SUFFIXES) for k in changed)
    for k in changed:
        assert torch.equal(refs["sharp_w"][k], refs["plain_w"][k] * 4.0)


def test_twin_distance_is_a_fair_floor_on_the_sharp_set(refs):
    """the premise that 1e-2 is a meaningful bound on the sharp set: gain 4 does not move the f16-operand floor"""
    for b in CHECKED:
        e4, e1 = refs["sharp"]["e"][b], refs["plain"]["e"][b]
        print(f"[fwd-ref] T={FRAMES[b]}: e sharp {e4:.3e}  plain {e1:.3e}")
        assert 0.0 < e4 < 1e-2, (FRAMES[b], e4)
        assert 0.0 < e1 < 1e-2, (FRAMES[b], e1)
        assert max(e4, e1) < 2.0 * min(e4, e1), (FRAMES[b], e4, e1)


def test_planted_errors_stand_out_on_the_sharp_set_and_hide_on_the_plain_one(refs):
    audio, lens = refs["audio"], refs["lens"]
    bad = FR.planted(refs["sharp_w"], audio, lens, CHECKED)
    for b in CHECKED:
        n, bound = FRAMES[b], refs["sharp"]["bound"][b]
        d_pos = FR.maxdiff(bad["positions"][b], refs["sharp"]["lp"][b], n)
        d_last = FR.maxdiff(bad["last_frame"][b], refs["sharp"]["lp"][b], n - 1)     # all frames but the last
        print(f"[fwd-ref] sharp T={n}: positions off by one {d_pos:.3f}, last frame dropped {d_last:.3f}, bound (a) {bound:.3e}")
        assert d_pos >= 4.0 * bound, (n, d_pos, bound)
        assert d_last >= 4.0 * bound, (n, d_last, bound)
    # The gap: on the plain random weights a position off-by-one moves the log-probs by LESS than the 1e-2 every oracle
    # comparison grants.  If this ever fails the plain weights have become sensitive enough to the position term, and
    # the sharp set is no longer the only place where such an error shows.
    with FR.positions_off_by_one():
        lp, _ = R.forward(refs["plain_w"], audio, lens)
    for b in (2, 3):
        d = FR.maxdiff(lp[b], refs["plain"]["lp"][b], FRAMES[b])
        print(f"[fwd-ref] plain T={FRAMES[b]}: positions off by one {d:.4f}")
        assert 0.0 < d < 1e-2, (FRAMES[b], d)


def test_planted_errors_leave_the_module_as_it_was(refs):
    f0, c0 = R.rel_pos_emb, R.conformer_layer
    with FR.positions_off_by_one():
        assert torch.equal(R.rel_pos_emb(5), torch.roll(f0(5), 1, 0))
    with FR.last_frame_dropped():
        assert R.conformer_layer is not c0
    assert R.rel_pos_emb is f0 and R.conformer_layer is c0


def test_attention_rounding_twin_restates_the_oracle_layer(refs, monkeypatch):
    """forward_ref.attention_roundings swaps in a restated Conformer layer: with its float16 roundings switched off it must BE
    the oracle's layer (softmax written as exp / sum: float32 noise only), and with them it stays on the twin's floor"""
    for b in CHECKED:
        d = FR.maxdiff(refs["sharp"]["twin_att"][b], refs["sharp"]["lp"][b], FRAMES[b])
        print(f"[fwd-ref] T={FRAMES[b]}: twin with attention roundings vs fp32 {d:.3e} (e {refs['sharp']['e'][b]:.3e})")
        assert 0.0 < d < 1e-2, (FRAMES[b], d)
    monkeypatch.setattr(FR, "_h", lambda x: x)
    layer = R.conformer_layer
    with FR.attention_roundings():
        lp, _ = R.forward(refs["sharp_w"], refs["audio"], refs["lens"])
    assert R.conformer_layer is layer
    for b, n in enumerate(FRAMES):
        assert FR.maxdiff(lp[b], refs["sharp"]["lp"][b], n) <= 2e-5, n


def test_structured_condition_leaves_few_frames_out():
    """GPU test 5 asks for equal argmax wherever the fp32 top-1 / top-2 gap exceeds 4 e; at most 5 % of the frames may fall
    outside that condition -- here with the reference alone, on that test's clips."""
    w = R.structured_weights(SEED)
    lens = [FR.samples_for_frames(t) for t in FR.STRUCTURED_FRAMES]
    ref = FR.reference(w, FR.clips(lens, FR.STRUCTURED_AUDIO_SEED), lens)
    assert ref["t"] == FR.STRUCTURED_FRAMES
    for b, n in enumerate(ref["t"]):
        keep = FR.decided_frames(ref["lp"][b, :n], ref["e"][b])
        left_out = 1.0 - float(keep.float().mean())
        print(f"[fwd-ref] structured T={n}: e {ref['e'][b]:.3e}, bound (a) {ref['bound'][b]:.3e}, frames left out {left_out:.3f}")
        assert left_out <= 0.05, (n, left_out)
        # the twin itself decides those frames as fp32 does
        assert bool((ref["twin"][b, :n].argmax(-1) == ref["lp"][b, :n].argmax(-1))[keep].all())


def test_oracle_is_batch_invariant(refs):
    """why one padded oracle call can serve a ragged device batch"""
    for b in (0, 3):
        n = refs["lens"][b]
        one, t = R.forward(refs["sharp_w"], refs["audio"][b: b + 1, :n].contiguous(), [n])
        assert int(t[0]) == FRAMES[b]
        d = FR.maxdiff(one[0], refs["sharp"]["lp"][b], FRAMES[b])
        print(f"[fwd-ref] T={FRAMES[b]} alone vs in the padded batch: {d:.2e}")
        assert d <= 1e-5, (FRAMES[b], d)


def test_samples_for_frames_is_the_smallest_count():
    for t in (1, 2, 33, 376, 766):
        n = FR.samples_for_frames(t)
        assert R.sub_len(R.mel_frames(n)) == t
        assert n == 400 or R.sub_len(R.mel_frames(n - 160)) == t - 1
    assert R.sub_len(R.mel_frames(FR.MAX_SAMPLES)) == 766


# ------------------------------------------------------------------ the instrument of tests/test_gpu_layer_taps.py -------
# One wrong tensor in one layer: does the tap behind that layer show it?  Oracle against oracle, no kernel.

TELL_FRAMES = [33, 129]


@pytest.fixture(scope="module")
def tell(refs):
    """per kind ('telltale', and 'telltale_q' = what a precision-1 engine makes of it): the 46 x 17 power table and the
    taps' float16 floor on the 33- and 129-frame clips of the ladder"""
    rows = [FRAMES.index(t) for t in TELL_FRAMES]
    audio, lens = FR._rows_of(refs["audio"], refs["lens"], rows)
    w = FR.telltale_weights(refs["plain_w"])
    out = {"audio": audio, "lens": lens}
    for kind, wk in (("telltale", w), ("telltale_q", R.quantize_linear_weights(w))):
        power = FR.layer_power(wk, audio, lens, range(len(lens)))
        assert power["t"] == TELL_FRAMES
        out[kind] = {"w": wk, "power": power, "floor": FR.tap_floor(wk, audio, lens, taps=power["taps"])}
    return out


KINDS = ["telltale", "telltale_q"]


def test_telltale_weights_change_what_they_say(refs):
    sharp, tell_w = refs["sharp_w"], FR.telltale_weights(refs["plain_w"])
    gains = dict(FR.TELLTALE_GAINS)
    for k, t in tell_w.items():
        suffix = next((s for s in gains if k.endswith(s)), None)
        if k.startswith("encoder.pre_encode.out."):
            assert torch.equal(t, sharp[k] * FR.TELLTALE_OUT_GAIN), k
        elif k.endswith("batch_norm.running_var"):
            assert torch.equal(t, 1.0 + FR.TELLTALE_VAR_SPREAD * (sharp[k] - 1.0)) and float(t.min()) >= 1.0, k
        elif suffix is not None and k.startswith("encoder.layers."):
            assert torch.equal(t, sharp[k] * gains[suffix]), k
        else:
            assert torch.equal(t, sharp[k]), k
    assert len(FR.LAYER_SUFFIXES) == 39 and FR.UNOBSERVABLE in FR.LAYER_SUFFIXES
    assert len(FR.PLANTS) == 39 + 7


@pytest.mark.parametrize("kind", KINDS)
def test_single_layer_reevaluation_is_the_oracle(tell, kind):
    """a plant is ONE R.conformer_layer call on the oracle's own input to that layer: without a plant that call must give
    the oracle's tap bit for bit, or the table measures something else"""
    assert tell[kind]["power"]["reeval"] == [0.0] * R.N_LAYERS


@pytest.mark.parametrize("kind", KINDS)
def test_tap_bound_is_the_projects_own(tell, kind):
    """1.5 e_tap <= 1.5e-2 at every layer and 1.5 e <= 1e-2 on the log-probs: the bounds asserted on the device are the
    project's 1.5e-2 / 1e-2, not floors this weight set inflated.  (If a candidate set breaks this, change the set.)"""
    fl = tell[kind]["floor"]
    print(f"[tell-ref] {kind}: e {' / '.join(f'{e:.2e}' for e in fl['e'])}, e_tap per layer " + " ".join(f"{e * 1e3:.1f}" for e in fl["e_tap"])
          + f" (x 1e-3), e_sub {fl['e_sub']:.2e}")
    for l, e in enumerate(fl["e_tap"]):
        assert 0.0 < FR.FLOOR_K * e <= FR.TAP_BOUND, (l, e)
    assert fl["bound_tap"] == [FR.TAP_BOUND] * R.N_LAYERS
    assert fl["bound"] == [1e-2] * len(TELL_FRAMES), fl["e"]
    assert FR.FLOOR_K * fl["e_sub"] <= FR.SUB_BOUND


@pytest.mark.parametrize("kind", KINDS)
def test_every_plant_shows_at_its_layer_tap(tell, kind):
    """The power of test_gpu_layer_taps.py: each of the 38 observable tensors of a layer replaced by the next layer's, and
    each of the seven structural slips, in each of the 17 layers, moves that layer's tap by >= 4 bounds -- the factor
    _planted_check uses.  On sharp_weights this test fails (see test_sharp_weights_hide_a_wrong_vector_in_layer_0)."""
    D, bound = tell[kind]["power"]["D"], tell[kind]["floor"]["bound_tap"]
    ratios = sorted((d / bound[l], key, l) for key, row in D.items() if key != FR.BLIND for l, d in enumerate(row))
    assert len(ratios) == 45 * R.N_LAYERS
    for r, key, l in ratios[:5]:
        print(f"[tell-ref] {kind}: {key} in layer {l}: {r:.2f} bounds")
    low = [(key, l, round(r, 2)) for r, key, l in ratios if r < 4.0]
    assert not low, low


@pytest.mark.parametrize("kind", KINDS)
def test_key_bias_is_invisible_by_construction(tell, kind):
    """linear_k.bias adds u.b_k + q.b_k to every key's content score of a query row: one constant per row, which the
    softmax removes; the position term and the values never see it.  No output of the model depends on it (float32 noise
    only), so no test can hold it -- on these or any weights."""
    d = tell[kind]["power"]["D"][FR.BLIND]
    print(f"[tell-ref] {kind}: linear_k.bias of the next layer, per layer: max {max(d):.1e}")
    assert max(d) <= 1e-4, d


def test_sharp_weights_hide_a_wrong_vector_in_layer_0(refs, tell):
    """The gap the telltale set closes, kept so that nobody removes it as redundant: on sharp_weights layer 0's input is
    +-30, and some vector of layer 0 replaced by layer 1's moves the layer-0 tap by less than bound + the device's own
    distance (1.5e-2 + 1e-2) -- a device with that error could pass the tap that test_gpu_forward*.py do compare."""
    vectors = {k: p for k, p in FR.MISROUTES.items() if refs["sharp_w"]["encoder.layers.0." + k[len("next:"):]].numel() <= R.FF
               and k != FR.BLIND}                    # biases, LayerNorm / BatchNorm vectors, pos_bias_u / v [8, 64]
    assert len(vectors) == 26
    D = FR.layer_power(refs["sharp_w"], tell["audio"], tell["lens"], range(len(TELL_FRAMES)), plants=vectors, layers=[0])["D"]
    hidden = sorted((d[0], k) for k, d in D.items() if d[0] < FR.TAP_BOUND + 1e-2)
    print(f"[tell-ref] sharp weights, layer 0: {len(hidden)} of {len(D)} vectors hidden, smallest {hidden[:3]}")
    assert hidden
    same = {k: tell["telltale"]["power"]["D"][k][0] for _, k in hidden}
    assert min(same.values()) >= 4.0 * FR.TAP_BOUND, same


# ------------------------------------------------------------------ the instrument of tests/test_gpu_ort_layers.py ------
# Precision 2 (OrtMixed): every layer from the oracle's OWN layer input, the conv module cut out.  Oracle against oracle.

ORT_TAPS = ["sub", "c2p"] + [f"{k}{l}" for l in range(R.N_LAYERS) for k in ("layer", "lnc", "glu", "dw")]
ORT_OUT_PLANTS = [k for k in FR.PLANTS2 if FR.plant_shows_at_out(k) or FR.plant_shows_at_lnc(k)]
ORT_CHAIN_PLANTS = [k for k in FR.PLANTS2 if FR.plant_stage(k)]


@pytest.fixture(scope="module")
def ort(refs):
    """the OrtMixed oracle on the telltale_ort weights, 33- and 129-frame clips, and per layer and clip: the cut layer's
    bits against R.conformer_layer's, the twins' envelope, every plant's distance"""
    rows = [FRAMES.index(t) for t in TELL_FRAMES]
    audio, lens = FR._rows_of(refs["audio"], refs["lens"], rows)
    w = FR.telltale_ort_weights(refs["plain_w"])
    taps = FR._Keep(ORT_TAPS)
    lp, t = R.forward(w, audio, lens, ort=FR.OrtOps(), taps=taps)
    assert t.tolist() == TELL_FRAMES
    out = {"w": w, "audio": audio, "lens": lens, "lp": lp, "taps": taps, "cells": {}}
    for l in range(R.N_LAYERS):
        for b, n in enumerate(TELL_FRAMES):
            x = taps["sub"][b, :n] * R.D_MODEL ** 0.5 if l == 0 else taps[f"layer{l - 1}"][b, :n]
            true = {k: taps[f"{k}{l}"][b, :n] for k in ("layer", "lnc", "glu", "dw")}
            whole = FR.ort_layer(w, FR._p(l), x.unsqueeze(0), FR.OrtOps())
            seg = FR.ort_segments(w, l, x, true["dw"], FR.ort_twins(), ORT_OUT_PLANTS)
            call = R.conformer_layer(w, FR._p(l), x.unsqueeze(0), R.rel_pos_emb(n).unsqueeze(0), torch.zeros(1, n, dtype=torch.bool), R.OrtMixed())
            seg["restated"] = [FR._d(whole["out"], call), FR._d(whole["out"][0], true["layer"]), FR._d(whole["lnc"][0], true["lnc"]),
                               FR._d(whole["glu"][0], true["glu"]), FR._d(whole["dw"][0], true["dw"]), FR._d(seg["out"], true["layer"]),
                               FR._d(seg["lnc"], true["lnc"])]
            seg["stage"] = {}
            for key in ORT_CHAIN_PLANTS:
                stage = FR.plant_stage(key)
                wp, ops = FR.planted2(key, w, l)
                bad = FR.ort_stage(wp, FR._p(l), stage, true["lnc" if stage == "glu" else "glu"], ops)
                seg["stage"][key] = FR._d(bad, true[stage]) / (FR.STAGE_REL * float(true[stage].abs().max()))
            out["cells"][(l, n)] = seg
    return out


def test_ort_ops_without_options_are_the_oracle(refs, ort):
    """OrtOps() is R.OrtMixed() bit for bit; its float16-input twin is ort_floor.make_f16_input_ops's, its noise ort_floor.make_noise_ops's"""
    import ort_floor

    audio, lens = ort["audio"][:1, : ort["lens"][0]].contiguous(), ort["lens"][:1]
    assert torch.equal(R.forward(ort["w"], ort["audio"], ort["lens"], ort=R.OrtMixed())[0], ort["lp"])
    for mine, theirs in ((FR.OrtOps(f16_inputs=True), ort_floor.make_f16_input_ops(R)), (FR.OrtOps(noise=(1e-7, 1)), ort_floor.make_noise_ops(R, 1e-7, 1))):
        assert torch.equal(R.forward(ort["w"], audio, lens, ort=mine)[0], R.forward(ort["w"], audio, lens, ort=theirs)[0])


def test_telltale_ort_weights_change_the_three_conv_weights_only(refs):
    tell_w, ort_w = FR.telltale_weights(refs["plain_w"]), FR.telltale_ort_weights(refs["plain_w"])
    assert len(set(FR.ORT_CONV_GAINS)) == 3 and min(FR.ORT_CONV_GAINS) >= 1.0
    for k, t in ort_w.items():
        if k.startswith("encoder.layers.") and k.endswith(FR.ORT_CONVS):
            assert torch.equal(t, tell_w[k] * FR.ORT_CONV_GAINS[int(k.split(".")[2]) % 3]), k
        else:
            assert torch.equal(t, tell_w[k]), k
    for l in range(R.N_LAYERS):          # what the gains are for: a neighbour's int8 scale is never within a third
        for s in FR.ORT_CONVS:
            a, b = (float(R.quantize_weight_int8(ort_w[FR._p(i) + s])[1]) for i in (l, (l + 1) % R.N_LAYERS))
            assert max(a, b) / min(a, b) >= 4.0 / 3.0, (l, s, a, b)
    assert len(FR.ORT_PLANTS) == 9 and len(FR.PLANTS2) == 46 + 9 and len(ORT_CHAIN_PLANTS) == 18
    assert len([k for k in FR.PLANTS2 if FR.plant_shows_at_out(k)]) == 46 + 9 - 1 - 18 - 2


def test_cut_layer_restates_the_oracle_layer(ort):
    """ort_layer == R.conformer_layer under OrtMixed, bit for bit: called alone, against the oracle's own taps (layer output, lnc,
    GLU, dw), and with the oracle's dw handed over -- all 17 layers, both clips"""
    for cell, seg in ort["cells"].items():
        assert seg["restated"] == [0.0] * 7, (cell, seg["restated"])


def test_ort_segment_bounds_stay_below_the_tap_bound(ort):
    """e per segment, layer and clip (printed), and FLOOR_K e <= TAP_BOUND: the bound asserted on the device is below the
    project's 1.5e-2 everywhere.  (If a cell breaks this, change the weight set.)"""
    names = list(FR.ort_twins())
    for n in TELL_FRAMES:
        print(f"[ort-ref] T = {n}: e at lnc | at the layer output, x 1e-3, per layer (and which twin sets it)")
        for l in range(R.N_LAYERS):
            seg = ort["cells"][(l, n)]
            who = [max(names, key=lambda k: seg["rows"][k][i]) for i in (0, 1)]
            print(f"[ort-ref]   layer {l:2d}: {seg['e_lnc'] * 1e3:5.2f} ({who[0]}) | {seg['e_out'] * 1e3:5.2f} ({who[1]})")
    for cell, seg in ort["cells"].items():
        for e in (seg["e_lnc"], seg["e_out"]):
            assert 0.0 < FR.FLOOR_K * e <= FR.TAP_BOUND, (cell, e)


def test_every_ort_plant_shows_where_its_check_looks(ort):
    """The power of test_gpu_ort_layers.py, the ORACLE computing the wrong thing, in all 17 layers on both clips: a plant in front
    of lnc lies >= 4 bounds (bound = FLOOR_K e of that cell) from the oracle at lnc; every plant outside the cut-out chain (and
    not norm_conv's, whose only reader is the chain) >= 4 bounds at the layer output with the TRUE dw handed over; a plant inside
    the chain moves its exact stage's tensor by >= 100 stage bounds (1e-5 of range each)."""
    at_lnc, at_out, at_stage = [], [], []
    for (l, n), seg in ort["cells"].items():
        at_lnc += [(d[0] / (FR.FLOOR_K * seg["e_lnc"]), key, l, n) for key, d in seg["D"].items() if FR.plant_shows_at_lnc(key)]
        at_out += [(d[1] / (FR.FLOOR_K * seg["e_out"]), key, l, n) for key, d in seg["D"].items() if FR.plant_shows_at_out(key)]
        at_stage += [(r, key, l, n) for key, r in seg["stage"].items()]
    assert len(at_out) == 34 * R.N_LAYERS * 2 and len(at_stage) == 18 * R.N_LAYERS * 2 and len(at_lnc) == 23 * R.N_LAYERS * 2
    for name, rows, least in (("lnc", at_lnc, 4.0), ("layer output", at_out, 4.0), ("stage tensor", at_stage, 100.0)):
        rows.sort()
        for r, key, l, n in rows[:3]:
            print(f"[ort-ref] {name}: {key} in layer {l}, T = {n}: {r:.1f} bounds")
        low = [(key, l, n, round(r, 2)) for r, key, l, n in rows if r < least]
        assert not low, (name, low)
    worst = {k: min(r for r, key, _, _ in at_out if key == k) for k in FR.ORT_PLANTS if FR.plant_shows_at_out(k)}
    print("[ort-ref] pointwise_conv2's precision-2 plants, fewest bounds at the layer output:", {k: round(v, 1) for k, v in worst.items()})


def test_pre_encode_restatement_and_floor(ort):
    """ort_pre_encode on the oracle's conv.6 output is the oracle's encoder input bit for bit, and its bound is below TAP_BOUND"""
    for b, n in enumerate(TELL_FRAMES):
        fl = FR.ort_pre_encode_floor(ort["w"], ort["taps"]["c2p"][b, :n])
        assert torch.equal(fl["ref"], ort["taps"]["sub"][b, :n] * R.D_MODEL ** 0.5)
        print(f"[ort-ref] pre_encode.out T = {n}: e {fl['e']:.2e} {fl['rows']}")
        assert 0.0 < FR.FLOOR_K * fl["e"] <= FR.TAP_BOUND
