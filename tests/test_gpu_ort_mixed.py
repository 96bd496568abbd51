"""QV_PREC_ORT_MIXED on the GPU: the arithmetic onnxruntime runs on the reference's model file
(experiments/c2c-direct-mixed/run.py:1-9 -- MatMulNBits int4 + DynamicQuantizeLinear / ConvInteger on every Conv)
against its CPU restatement oracle/fastconformer_ref.py::OrtMixed, through the C ABI.

Two kinds of checks:
  * STAGE checks: the float32 tensor in front of a quantiser is read back from the device (qv_debug_forward_tap 3..9),
    the oracle runs that one Conv on it, and the device's own output tensor must equal the oracle's.  The integer part
    (quantised activations, int8 weights, int32 accumulation, float32 rescale + bias) has no tolerance to hide in: one
    wrong LSB is 4e-3 of the tensor's range; the bounds below are 1e-5 of it (Swish / sigmoid differ by an ulp or two
    between expf implementations, everything else is expected to be bit-identical and the match rate is printed).
  * END-TO-END: log-probs against the oracle.  The oracle differs from ITSELF by ~0.05 max / ~0.012 rms when only the
    float32 summation order changes (1 vs 16 threads; profiles/archive/r03_a_ort_noise_floor.json), because every
    DynamicQuantizeLinear is a rounding discontinuity; the bound here is that floor with head room, and the f16-weight
    path (QV_PREC_MIXED_INT4_INT8) must be several times further away.
"""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ort_floor import FLOOR_K, _assert_on_the_floor  # noqa: F401
from synth import synth_audio

pytestmark = pytest.mark.gpu

SEED = 7
LENS = [48000, 30000, 17777]


@pytest.fixture(scope="module")
def setup():
    os.environ["QVERSE_DEBUG_TAPS"] = "1"
    from offline_tarteel_amd.engine import Engine
    from oracle import fastconformer_ref as R

    torch.set_num_threads(min(16, torch.get_num_threads()))
    audio = torch.from_numpy(synth_audio(3, 48000))
    for b, n in enumerate(LENS):
        audio[b, n:] = 0
    w = R.random_weights(SEED)
    eng = Engine(device=0, with_model=True, seed=SEED, precision=2, max_batch=4, max_samples=80000)
    lp, t = eng.forward(audio.cuda().contiguous(), LENS)
    torch.cuda.synchronize()
    tm = [n // 160 + 1 for n in LENS]
    sl = lambda x: (x + 2 - 3) // 2 + 1  # noqa: E731
    l1 = [sl(x) for x in tm]
    l2 = [sl(x) for x in l1]
    l3 = [sl(x) for x in l2]
    assert l3 == t
    yield dict(eng=eng, audio=audio, lp=lp, t=t, w=w, R=R, tm=tm, l1=l1, l2=l2, l3=l3, ort=R.OrtMixed())
    eng.close()
    os.environ.pop("QVERSE_DEBUG_TAPS", None)


def _report(name, got, want, rel):
    got, want = got.float(), want.float()
    scale = float(want.abs().max())
    d = float((got - want).abs().max())
    same = float((got == want).float().mean())
    print(f"[ort-stage] {name}: max|d| {d:.3e} of range {scale:.3e}, bit-identical {same:.6f}")
    assert d <= rel * scale, (name, d, scale, same)


def test_frontend_integer_stages(setup):
    """normalised mel -> conv.0 + ReLU -> conv.2 | -> conv.3 + ReLU | -> conv.5 | -> conv.6 + ReLU, each stage on the
    DEVICE's own input tensor."""
    eng, w, ort = setup["eng"], setup["w"], setup["ort"]
    tm, l2, l3 = setup["tm"], setup["l2"], setup["l3"]
    B = len(LENS)
    pe = "encoder.pre_encode."
    mel = eng.forward_tap(0, 0, (B, max(tm), 80)).cpu()
    c1 = eng.forward_tap(6, 0, (B, max(l2), 20, 256)).cpu()
    c1p = eng.forward_tap(7, 0, (B, max(l2), 20, 256)).cpu()
    c2 = eng.forward_tap(8, 0, (B, max(l3), 10, 256)).cpu()
    c2p = eng.forward_tap(9, 0, (B, max(l3), 10, 256)).cpu()
    for b in range(B):
        x = mel[b, : tm[b]].unsqueeze(0).unsqueeze(0)                                   # [1,1,Tm,80]
        y = F.relu(ort.conv(w, pe + "conv.0.weight", x, pe + "conv.0.bias", F.conv2d, stride=2, padding=1))
        y = ort.conv(w, pe + "conv.2.weight", y, pe + "conv.2.bias", F.conv2d, stride=2, padding=1, groups=256)
        _report(f"conv.0+conv.2[{b}]", c1[b, : l2[b]], y[0].permute(1, 2, 0), 1e-6)
        x = c1[b, : l2[b]].permute(2, 0, 1).unsqueeze(0).contiguous()                   # [1,256,T2,20]
        y = F.relu(ort.conv(w, pe + "conv.3.weight", x, pe + "conv.3.bias", F.conv2d))
        _report(f"conv.3[{b}]", c1p[b, : l2[b]], y[0].permute(1, 2, 0), 1e-6)
        x = c1p[b, : l2[b]].permute(2, 0, 1).unsqueeze(0).contiguous()
        y = ort.conv(w, pe + "conv.5.weight", x, pe + "conv.5.bias", F.conv2d, stride=2, padding=1, groups=256)
        _report(f"conv.5[{b}]", c2[b, : l3[b]], y[0].permute(1, 2, 0), 1e-6)
        x = c2[b, : l3[b]].permute(2, 0, 1).unsqueeze(0).contiguous()
        y = F.relu(ort.conv(w, pe + "conv.6.weight", x, pe + "conv.6.bias", F.conv2d))
        _report(f"conv.6[{b}]", c2p[b, : l3[b]], y[0].permute(1, 2, 0).half().float(), 1e-6)   # stored as f16 (feeds the int4 Linear)


def test_conv0_on_the_matrix_pipe_equals_the_valu_kernel(setup):
    """QV_KV_ORT_SUB 1 (five v_mfma_f32_32x32x2_f32 per tile on the integer-valued operands, four channel groups per block)
    against 0 (VALU, a block per channel group): every sum is an exact integer, so conv.0 + conv.2's output, the ranges
    folded for the next quantisers and therefore the log-probs are bit-identical."""
    eng = setup["eng"]
    l2 = setup["l2"]
    dev = setup["audio"].cuda().contiguous()
    got = {}
    try:
        for var in (0, 1):
            eng.kernel_variant(1, var)
            lp, t = eng.forward(dev, LENS)
            torch.cuda.synchronize()
            got[var] = (eng.forward_tap(6, 0, (len(LENS), max(l2), 20, 256)).clone(), lp.clone(), t)
    finally:
        eng.kernel_variant(1, -1)
    assert got[0][2] == got[1][2] == setup["t"]
    for b in range(len(LENS)):
        assert torch.equal(got[0][0][b, : l2[b]], got[1][0][b, : l2[b]]), b
        assert torch.equal(got[0][1][b, : setup["t"][b]], got[1][1][b, : setup["t"][b]]), b


@pytest.mark.parametrize("layer", [0, 8, 16])
def test_conv_module_stages(setup, layer):
    """norm_conv output -> pointwise_conv1 + GLU | -> depthwise_conv + BatchNorm + Swish, on the device's own inputs."""
    eng, w, ort, T = setup["eng"], setup["w"], setup["ort"], setup["t"]
    B = len(LENS)
    c = f"encoder.layers.{layer}.conv."
    lnc = eng.forward_tap(3, layer, (B, max(T), 512)).cpu()
    glu = eng.forward_tap(4, layer, (B, max(T), 512)).cpu()
    dw = eng.forward_tap(5, layer, (B, max(T), 512)).cpu()
    for b in range(B):
        x = lnc[b, : T[b]].t().unsqueeze(0).contiguous()                                # [1,512,T]
        y = F.glu(ort.conv(w, c + "pointwise_conv1.weight", x, c + "pointwise_conv1.bias", F.conv1d), dim=1)
        _report(f"L{layer} pw1+GLU[{b}]", glu[b, : T[b]], y[0].t(), 1e-5)
        x = glu[b, : T[b]].t().unsqueeze(0).contiguous()
        y = ort.conv(w, c + "depthwise_conv.weight", x, c + "depthwise_conv.bias", F.conv1d, padding=4, groups=512)
        y = F.batch_norm(y, w[c + "batch_norm.running_mean"], w[c + "batch_norm.running_var"], w[c + "batch_norm.weight"],
                         w[c + "batch_norm.bias"], False, 0.0, 1e-5)
        y = y * torch.sigmoid(y)
        _report(f"L{layer} dw+BN+Swish[{b}]", dw[b, : T[b]], y[0].t(), 1e-5)


def test_whole_layer_and_head_on_device_inputs(setup):
    """one whole Conformer layer (covers pointwise_conv2's residual epilogue) and the CTC head, each from the device's own
    input: the Linear layers run f16-operand GEMMs here, so the bound is the f16 path's, with room for an LSB flip."""
    eng, w, ort, R, T = setup["eng"], setup["w"], setup["ort"], setup["R"], setup["t"]
    B = len(LENS)
    x0 = eng.forward_tap(1, 0, (B, max(T), 512)).cpu()
    x1 = eng.forward_tap(2, 0, (B, max(T), 512)).cpu()
    xe = eng.forward_tap(2, 16, (B, max(T), 512)).cpu()
    head = "ctc_decoder.decoder_layers.0."
    for b in range(B):
        t = T[b]
        pos = R.rel_pos_emb(t).unsqueeze(0)
        pad = torch.zeros(1, t, dtype=torch.bool)
        y = R.conformer_layer(w, "encoder.layers.0.", x0[b: b + 1, :t], pos, pad, ort)
        d = float((y[0] - x1[b, :t]).abs().max())
        print(f"[ort-stage] layer0[{b}]: max|d| {d:.3e} (values ~ +-3)")
        assert d <= 5e-2, d
        lg = ort.conv(w, head + "weight", xe[b: b + 1, :t].transpose(1, 2), head + "bias", F.conv1d).transpose(1, 2)
        want = torch.log_softmax(lg, -1)[0]
        got = setup["lp"][b, :t].cpu()
        _report(f"head[{b}]", got, want, 2e-6)


def test_logprobs_against_the_oracle_and_its_noise_floor(setup):
    """End to end against the oracle, judged against the ORACLE'S OWN reproducibility on the same clips (ort_floor.py):
    the device may be at most FLOOR_K x as far from the oracle as the oracle is from itself when only the float32
    summation order / one ulp of its Linear inputs change -- not a fixed number that a 4x regression would pass."""
    from ort_floor import delta, oracle_floor

    R, w, T = setup["R"], setup["w"], setup["t"]
    lp_ref, t_ref = R.forward(w, setup["audio"], LENS, ort=R.OrtMixed())
    assert t_ref.tolist() == T
    got = setup["lp"].cpu()
    floor = oracle_floor(R, w, setup["audio"], LENS, lp_ref, T)
    _assert_on_the_floor("random weights, 3 ragged clips", delta(got, lp_ref, T), floor)
    mx, rms, same = delta(got, lp_ref, T)
    for b, n in enumerate(T):
        assert torch.allclose(got[b, :n].exp().sum(-1), torch.ones(n), atol=1e-4)
    # the f16-arithmetic mixed path is a different model from this one
    from offline_tarteel_amd.engine import Engine

    eng1 = Engine(device=0, with_model=True, seed=SEED, precision=1, max_batch=4, max_samples=80000)
    try:
        lp1, _ = eng1.forward(setup["audio"].cuda().contiguous(), LENS)
        d1 = delta(lp1, lp_ref, T)
        print(f"[ort-e2e] hip_mixed (W4A16/W8A16) vs OrtMixed: max {d1[0]:.4f} rms {d1[1]:.5f}")
        assert d1[1] > 1.5 * rms
    finally:
        eng1.close()


@pytest.mark.parametrize("weight_set", ["structured", "damped"])
def test_weight_sets_stay_on_their_own_floor(tmp_path, weight_set):
    """The same judgement on other weight sets (tools/ort_floor_table.py writes the table, profiles/r06_*_ort_floor_table.json):
    `structured` = rank-16 + noise matrices with a peaked blank-biased CTC head (fastconformer_ref.structured_weights) -- i.i.d.
    weights are the worst case for rounding-boundary flips, and where the floor moves the device has to follow it (the bound is
    relative); `damped` = the residual branches' output matrices x0.25 and the head x0.1 (damped_weights) -- the set whose floor
    lies BELOW north_star's 1e-2, where the device is held to 1e-2 ABSOLUTE as north_star states it."""
    import importlib.util
    import sys
    from pathlib import Path

    from offline_tarteel_amd.engine import Engine
    from oracle import fastconformer_ref as R
    from ort_floor import delta, oracle_floor

    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("convert_weights", str(root / "tools" / "convert_weights.py"))
    C = importlib.util.module_from_spec(spec)
    sys.modules["convert_weights"] = C
    spec.loader.exec_module(C)
    w = (R.structured_weights if weight_set == "structured" else R.damped_weights)(SEED)
    shapes = C.weight_shapes(C._lib())
    path = tmp_path / f"{weight_set}.qvw"
    C.write_qvw(path, {k: w[k].numpy() for k in shapes})
    lens = [48000, 30000]
    audio = torch.from_numpy(synth_audio(2, 48000, seed=5))
    audio[1, lens[1]:] = 0
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lp_ref, t_ref = R.forward(w, audio, lens, ort=R.OrtMixed())
    T = t_ref.tolist()
    floor = oracle_floor(R, w, audio, lens, lp_ref, T)
    peak = float(torch.cat([lp_ref[b, : T[b]].exp().max(-1).values for b in range(2)]).mean())
    print(f"[ort-e2e] {weight_set} weights: mean max-probability {peak:.3f}")
    if weight_set == "damped":
        assert floor["max"] < 1e-2, floor      # the point of this set: the arithmetic reproduces itself below north_star's tolerance
    eng = Engine(device=0, with_model=True, weights_path=str(path), precision=2, max_batch=2, max_samples=48000)
    try:
        lp, t = eng.forward(audio.cuda().contiguous(), lens)
        assert t == T
        got = delta(lp, lp_ref, T)
        _assert_on_the_floor(f"{weight_set} weights", got, floor)
        if floor["max"] < 1e-2:
            assert got[0] <= 1e-2, (weight_set, got, floor)     # north_star: CTC log-probs within 1e-2, absolute
    finally:
        eng.close()


def test_the_integer_chain_from_the_audio(setup):
    """The stage tests above start every stage from the DEVICE's own input tensor: they pin each stage, not the chain.
    Here both sides run the whole chain from the audio and the stage tensors are compared in place: conv.2 / conv.3 /
    conv.5 / conv.6 outputs and, for layers 0 and 8, norm_conv -> pointwise_conv1 + GLU -> depthwise + BN + Swish.  A
    stage's output moves in steps of its quantiser's LSB (s_x * s_w per unit of the integer accumulator), so `differs`
    counts elements further apart than a quarter of the smallest such step seen in the tensor, i.e. elements whose
    integer accumulators are not the same.  Reported per stage: the fraction that differs and the largest difference
    relative to the tensor's range; the first stage with a difference is named.  What is asserted: the first integer
    stage (conv.0 + conv.2, fed by log-mel features that agree to ~1e-4) has < 2 % of its elements off and nothing
    further than 2 % of its range, and no later stage of the subsampling stack is further than 5 % of its range --
    differences enter through rounding-boundary flips of individual activations and stay local."""
    eng, R, w = setup["eng"], setup["R"], setup["w"]
    tm, l2, l3, T = setup["tm"], setup["l2"], setup["l3"], setup["t"]
    B = len(LENS)
    taps = {}
    R.forward(w, setup["audio"], LENS, ort=R.OrtMixed(), taps=taps)
    stages = [("mel", eng.forward_tap(0, 0, (B, max(tm), 80)).cpu(), taps["mel"], tm),
              ("conv.0+conv.2", eng.forward_tap(6, 0, (B, max(l2), 20, 256)).cpu(), taps["c1"], l2),
              ("conv.3+ReLU", eng.forward_tap(7, 0, (B, max(l2), 20, 256)).cpu(), taps["c1p"], l2),
              ("conv.5", eng.forward_tap(8, 0, (B, max(l3), 10, 256)).cpu(), taps["c2"], l3),
              ("conv.6+ReLU", eng.forward_tap(9, 0, (B, max(l3), 10, 256)).cpu(), taps["c2p"].half().float(), l3)]
    for layer in (0, 8):
        stages += [(f"L{layer} norm_conv", eng.forward_tap(3, layer, (B, max(T), 512)).cpu(), taps[f"lnc{layer}"], T),
                   (f"L{layer} pw1+GLU", eng.forward_tap(4, layer, (B, max(T), 512)).cpu(), taps[f"glu{layer}"], T),
                   (f"L{layer} dw+BN+Swish", eng.forward_tap(5, layer, (B, max(T), 512)).cpu(), taps[f"dw{layer}"], T)]
    first = None
    table = {}
    for name, got, want, lens in stages:
        worst_frac, worst_rel = 0.0, 0.0
        for b in range(B):
            g, r = got[b, : lens[b]].float(), want[b, : lens[b]].float()
            rng = float(r.abs().max()) or 1.0
            d = (g - r).abs()
            worst_frac = max(worst_frac, float((d > 2e-4 * rng).float().mean()))
            worst_rel = max(worst_rel, float(d.max()) / rng)
        table[name] = (worst_frac, worst_rel)
        if first is None and name != "mel" and worst_frac > 0:
            first = name
        print(f"[ort-chain] {name}: {100 * worst_frac:.3f} % of the elements differ, largest difference {worst_rel:.2e} of the range")
    print(f"[ort-chain] first stage with a difference: {first}")
    assert table["mel"][1] <= 1e-3
    assert table["conv.0+conv.2"][0] <= 0.02 and table["conv.0+conv.2"][1] <= 0.02, table["conv.0+conv.2"]
    for name in ("conv.3+ReLU", "conv.5", "conv.6+ReLU"):
        assert table[name][1] <= 0.05, (name, table[name])


def test_batch_invariance_is_exact(setup):
    """the activation ranges are per utterance: an utterance alone == the same utterance inside a ragged batch, bit for bit
    (the reference quantises per call and feeds batch 1)."""
    eng, audio = setup["eng"], setup["audio"]
    for b in (1, 2):
        n = LENS[b]
        lp1, t1 = eng.forward(audio[b: b + 1, :n].cuda().contiguous(), [n])
        assert t1[0] == setup["t"][b]
        assert torch.equal(lp1[0, : t1[0]], setup["lp"][b, : t1[0]])


def test_predict_batch_runs_the_whole_path(setup, oracle):
    eng = setup["eng"]
    res = eng.predict_batch(setup["audio"].cuda().contiguous(), LENS)
    for i, n in enumerate(setup["t"]):
        want = oracle.predict_logprobs(setup["lp"][i, :n].cpu().numpy())
        assert res[i]["greedy_ids"] == want["greedy_ids"]
        assert (res[i]["surah"], res[i]["ayah"], res[i]["ayah_end"], res[i]["source"]) == (
            want["surah"], want["ayah"], want["ayah_end"], want["source"])


def test_configs2_batch256_ort_mixed_vs_oracle_sample():
    """BASELINE configs[2] at full size (256 clips x 10 s) in the reference's arithmetic: two utterances of the batch
    against the oracle (noise-floor bound), and a third against itself run alone (exact)."""
    from offline_tarteel_amd.engine import Engine
    from oracle import fastconformer_ref as R

    n = 160000
    audio = torch.from_numpy(synth_audio(256, n, seed=31))
    eng = Engine(device=0, with_model=True, seed=20260630, precision=2, max_batch=256, max_samples=n)
    try:
        a = audio.cuda().contiguous()
        lp, T = eng.forward(a, [n] * 256)
        torch.cuda.synchronize()
        assert T == [126] * 256
        one, _ = eng.forward(a[200:201].contiguous(), [n])
        assert torch.equal(one[0], lp[200])
        from ort_floor import delta, oracle_floor

        w = R.random_weights(20260630)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        for b in (0, 255):
            ref, _ = R.forward(w, audio[b: b + 1], [n], ort=R.OrtMixed())
            floor = oracle_floor(R, w, audio[b: b + 1], [n], ref, [126], one_thread=False, seeds=(1, 2, 3))
            _assert_on_the_floor(f"B=256 utt {b}", delta(lp[b: b + 1], ref, [126]), floor)
        res = eng.predict_batch(a, [n] * 256, want_text=False)
        assert len(res) == 256 and all(r["t_frames"] == 126 for r in res)
    finally:
        eng.close()


def test_prequantised_file_in_the_export_form_runs_on_its_own_integers(tmp_path):
    """VERDICT r2 items 1(c) + 8: a full-size model written the way the reference's export is described (torch-export
    scopes, MatMulNBits WITH zero points, DynamicQuantizeLinear -> ConvInteger chains, STFT baked in; tests/synth_onnx.py)
    -> tools/convert_weights.py --onnx -> precision 2.  The file is marked pre-quantised: Linear weights run as the
    dequantised MatMulNBits values, Conv weights go back on the file's integers with the file's scale.  Checked against
    the oracle given the same dequantised values and scales; the same values WITHOUT the marker are re-quantised onto the
    engine's own symmetric int4 grid and must land measurably further away."""
    import importlib.util
    import sys
    from pathlib import Path

    from offline_tarteel_amd.engine import Engine
    from oracle import fastconformer_ref as R
    from synth_onnx import export_like_model

    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("convert_weights", str(root / "tools" / "convert_weights.py"))
    C = importlib.util.module_from_spec(spec)
    sys.modules["convert_weights"] = C
    spec.loader.exec_module(C)
    lib = C._lib()
    shapes = C.weight_shapes(lib)
    w0 = C.random_weights(lib, shapes, SEED)
    onnx_path = tmp_path / "export_like.onnx"
    deq, scales = export_like_model(w0, onnx_path)
    sd, meta = C.onnx_state_dict(str(onnx_path), shapes, verbose=False, with_meta=True)
    marked, plain = tmp_path / "marked.qvw", tmp_path / "plain.qvw"
    C.write_qvw(marked, {k: sd[k] for k in shapes}, C.prequantised_extras(meta))
    C.write_qvw(plain, {k: sd[k] for k in shapes})
    wt = {k: torch.from_numpy(np.ascontiguousarray(deq[k], dtype=np.float32).reshape(shapes[k])) for k in shapes}
    lens = [32000, 17777]
    audio = torch.from_numpy(synth_audio(2, 32000))
    audio[1, lens[1]:] = 0
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lp_ref, t_ref = R.forward(wt, audio, lens, ort=R.OrtMixed(int4_linears=False, conv_scales=scales))
    T = t_ref.tolist()

    from ort_floor import delta, oracle_floor

    def run(path):
        eng = Engine(device=0, with_model=True, weights_path=str(path), precision=2, max_batch=2, max_samples=32000)
        try:
            lp, t = eng.forward(audio.cuda().contiguous(), lens)
            assert t == T
            return delta(lp, lp_ref, T)
        finally:
            eng.close()

    got = run(marked)
    mx, rms = got[:2]
    mx_p, rms_p = run(plain)[:2]
    floor = oracle_floor(R, wt, audio, lens, lp_ref, T, int4_linears=False, conv_scales=scales)
    # A marked file is never re-quantised, and it does not silently fall back to f16 either: under precisions 1
    # and 2 every Linear weight runs W4A16 on the FILE's own MatMulNBits grid (its integers, its zero points, its scale
    # rounded to f16), which qv_weights_info reports; precision 0 runs the dequantised values as f16 operands.
    outs, infos = {}, {}
    for prec, path in ((0, marked), (1, marked), (1, plain)):
        eng = Engine(device=0, with_model=True, weights_path=str(path), precision=prec, max_batch=2, max_samples=32000)
        try:
            lp, t = eng.forward(audio.cuda().contiguous(), lens)
            outs[(prec, path.name)] = lp.cpu()
            infos[(prec, path.name)] = eng.weights_info()
        finally:
            eng.close()

    def valid(lp):   # the frames that exist; rows t >= T[b] are qv_forward's zero padding (checked below)
        return torch.cat([lp[b, : T[b]].flatten() for b in range(len(T))])

    print("[ort-prequant]", infos)
    assert "103 Linear tensors on the file's own int4 grid" in infos[(1, "marked.qvw")] and ", 0 as dequantised" in infos[(1, "marked.qvw")]
    assert "quantised by the engine" in infos[(1, "plain.qvw")]
    same_values = float((valid(outs[(0, "marked.qvw")]) - valid(outs[(1, "marked.qvw")])).abs().max())
    requantised = float((valid(outs[(0, "marked.qvw")]) - valid(outs[(1, "plain.qvw")])).abs().max())
    print(f"[ort-prequant] precision 1 vs precision 0 on the marked file: max {same_values:.4f}; re-quantised (unmarked): {requantised:.4f}")
    assert 0.0 < same_values <= 2e-2          # the same weight VALUES: f16 scale rounding and W4A16 vs f16 operand rounding only
    assert requantised > 5 * same_values      # a second quantisation on another grid is a different model
    for lp in outs.values():
        assert all(bool((lp[b, T[b]:] == 0).all()) for b in range(len(T)))
    print(f"[ort-prequant] marked file vs oracle: max {mx:.4f} rms {rms:.5f}; unmarked (re-quantised): max {mx_p:.4f} rms {rms_p:.5f}")
    _assert_on_the_floor("marked file", got, floor)
    assert rms_p > 1.5 * rms, (rms_p, rms)


def test_edge_shapes_one_frame_thirty_seconds_and_silence():
    """precision 2 on the shapes the fp16 path is tested on: the shortest legal clip (400 samples -> 1 encoder frame:
    every per-utterance range is taken over a handful of values), a 30 s clip (T = 376: several query groups, the long
    CTC kernel), an all-zero clip (degenerate ranges: scale 0 -> the ONNX rule x_q = 0, zero point 0) and a near-silent
    one -- ragged in one batch, against each utterance run alone (exact) and against the oracle (noise-floor bound).
    Exact digital silence is NOT compared with the oracle: every mel frame is the same constant, the per-feature std is 0
    and (x - mean) / (0 + 1e-5) amplifies the rounding of the MEAN by 1e5 -- zero here (f64 statistics), O(1) noise in
    the oracle's float32 sum; no two implementations agree there, the reference's included."""
    from offline_tarteel_amd.engine import Engine
    from oracle import fastconformer_ref as R

    lens = [400, 480000, 16000, 48000, 16000]
    audio = torch.from_numpy(synth_audio(5, 480000, seed=91))
    for b, n in enumerate(lens):
        audio[b, n:] = 0
    audio[2] = 0                                         # silence
    audio[4, :16000] *= 1e-3                             # near silence
    eng = Engine(device=0, with_model=True, seed=SEED, precision=2, max_batch=5, max_samples=480000)
    try:
        a = audio.cuda().contiguous()
        lp, T = eng.forward(a, lens)
        torch.cuda.synchronize()
        assert T == [1, 376, 13, 38, 13]
        assert all(bool(torch.isfinite(lp[b, : T[b]]).all()) for b in range(5))
        for b in range(5):
            one, t1 = eng.forward(a[b: b + 1, : lens[b]].contiguous(), [lens[b]])
            assert t1[0] == T[b] and torch.equal(one[0, : T[b]], lp[b, : T[b]]), b
        w = R.random_weights(SEED)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        from ort_floor import delta, oracle_floor

        for b in (0, 4, 3, 1):
            one = audio[b: b + 1, : lens[b]].contiguous()
            ref, tr = R.forward(w, one, [lens[b]], ort=R.OrtMixed())
            assert int(tr[0]) == T[b]
            # a clip of ONE frame has a handful of values per quantiser: sub-ulp noise rarely flips any of them (the floor
            # reads ~3e-3 or exactly 0), while the f16 rounding of the Linear inputs -- the device's design point, equal
            # to the other perturbations on ordinary clips (profiles/archive/r03_a_ort_noise_floor.json) -- does.  The edge
            # shapes are therefore judged against the envelope that includes that row.
            floor = oracle_floor(R, w, one, [lens[b]], ref, [T[b]], one_thread=False, seeds=(1, 2, 3), f16_inputs=True)
            _assert_on_the_floor(f"edge utt {b} (T = {T[b]})", delta(lp[b: b + 1], ref, [T[b]]), floor)
        res = eng.predict_batch(a, lens)
        assert [r["t_frames"] for r in res] == T
    finally:
        eng.close()
