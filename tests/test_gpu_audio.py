"""a15 on the GPU: qv_upfirdn (the polyphase FIR behind the TTA wrapper's speed perturbation,
experiments/c2c-direct-mixed-tta/run.py:60-71) against scipy.signal.resample_poly -- the very
call the reference makes -- bit for bit, through the C ABI."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from offline_tarteel_amd.engine import Engine

    e = Engine(device=0, with_model=False, max_batch=2, max_samples=16000)
    yield e
    e.close()


@pytest.mark.parametrize("n_in,up,down", [(160000, 9, 10), (160000, 11, 10), (48001, 9, 10), (777, 11, 10), (5, 9, 10),
                                          (1, 11, 10), (44100, 160, 441), (480000, 11, 10), (1000, 18, 20)])
def test_upfirdn_equals_scipy_resample_poly(eng, n_in, up, down):
    from scipy.signal import resample_poly

    rng = np.random.default_rng(n_in + up)
    x = (rng.standard_normal(n_in) * 0.3).astype(np.float32)
    want = resample_poly(x, up, down)
    got = eng.resample_poly(torch.from_numpy(x).cuda(), up, down).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_speed_perturb_factors(eng):
    from scipy.signal import resample_poly

    from synth import synth_audio

    x = synth_audio(1, 80000, seed=9)[0]
    d = torch.from_numpy(x).cuda()
    assert eng.speed_perturb(d, 1.0) is d
    for f in (0.9, 1.1):
        want = resample_poly(x, int(f * 10), 10).astype("float32")   # tta/run.py:69-71
        assert np.array_equal(eng.speed_perturb(d, f).cpu().numpy(), want)
    # identity ratio after gcd reduction
    assert torch.equal(eng.resample_poly(d, 10, 10), d)


@pytest.mark.parametrize("up,down", [(9, 10), (11, 10), (160, 441), (1, 3)])
def test_batched_resampler_equals_scipy_row_by_row(eng, up, down):
    """qv_upfirdn_batch (round 6): many ragged rows in ONE launch, optionally picked out of a larger matrix (src_rows), written
    zero-padded into the engine's input layout -- every row bit-identical to scipy.signal.resample_poly of that row."""
    from scipy.signal import resample_poly

    rng = np.random.default_rng(up * 1000 + down)
    lens = [44100, 30000, 1, 7, 12345, 44099, 2205]
    x = np.zeros((len(lens) + 2, max(lens) + 13), dtype=np.float32)       # pitch > longest row, two rows never used
    for r, n in enumerate(lens):
        x[r + 1, :n] = (rng.standard_normal(n) * 0.3).astype(np.float32)
    src = [r + 1 for r in range(len(lens))]
    order = [3, 0, 6, 2, 5, 1, 4]                                          # output rows in another order than the source rows
    y, n_out = eng.resample_rows(torch.from_numpy(x).cuda(), [lens[i] for i in order], up, down, src_rows=[src[i] for i in order])
    y = y.cpu().numpy()
    for k, i in enumerate(order):
        want = resample_poly(x[src[i], : lens[i]], up, down)
        assert n_out[k] == len(want)
        assert np.array_equal(y[k, : n_out[k]].view(np.uint32), want.view(np.uint32)), (up, down, lens[i])
        assert not y[k, n_out[k]:].any()                                   # zero padding up to the pitch
    # without src_rows: row r of the input
    y2, n2 = eng.resample_rows(torch.from_numpy(x[1:1 + len(lens)]).cuda(), lens, up, down, out_pitch=max(n_out) + 5)
    y2 = y2.cpu().numpy()
    for r, n in enumerate(lens):
        want = resample_poly(x[r + 1, :n], up, down)
        assert np.array_equal(y2[r, : n2[r]].view(np.uint32), want.view(np.uint32)) and not y2[r, n2[r]:].any()


@pytest.mark.parametrize("channels", [2, 3, 6])
def test_device_mixdown_equals_numpy_mean(eng, channels):
    rng = np.random.default_rng(channels)
    frames = [1000, 1, 777]
    x = np.zeros((3, max(frames) * channels), dtype=np.float32)
    for r, n in enumerate(frames):
        x[r, : n * channels] = (rng.standard_normal(n * channels) * 0.5).astype(np.float32)
    y = eng.mixdown_rows(torch.from_numpy(x).cuda(), frames, channels).cpu().numpy()
    for r, n in enumerate(frames):
        want = x[r, : n * channels].reshape(-1, channels).mean(axis=1)
        assert np.array_equal(y[r, :n].view(np.uint32), want.astype(np.float32).view(np.uint32))
        assert not y[r, n:].any()


def _wav(path, x, sr, ch, kind):
    import struct

    import audio_ref as A

    if kind in ("pcm24", "u8", "ext_pcm16"):
        bits = {"pcm24": 24, "u8": 8, "ext_pcm16": 16}[kind]
        return path.write_bytes(A.wav_bytes(A.pcm_bytes(A.quantise(x, bits), bits), sr, ch, 1, bits, extensible=kind.startswith("ext_")))
    if kind == "f64":
        return path.write_bytes(A.wav_bytes(x.astype("<f8").tobytes(), sr, ch, 3, 64))
    if kind == "pcm16":
        pcm = np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2").tobytes()
        tag, bits = 1, 16
    else:
        pcm = x.astype("<f4").tobytes()
        tag, bits = 3, 32
    align = ch * bits // 8
    hdr = b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, tag, ch, sr, sr * align, align, bits)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(pcm)) + pcm)


def test_device_ingest_equals_host_load_audio(eng, tmp_path):
    """audio.load_audio_device: containers parsed on the host, mix-down + resampling to 16 kHz on the GPU (44.1 kHz stereo
    -> 160/441, 48 kHz -> 1/3, 22.05 kHz 3-channel, 16 kHz mono untouched) -- the same float32 samples load_audio() returns,
    bit for bit, zero-padded to the longest clip, in the order of the paths.  The second line of files: 8 channels (numpy's
    eight-sum order), 24-bit, 8-bit at 11,025 Hz (640/441: the LDS kernel's largest footprint), float64, EXTENSIBLE, and
    44,056 Hz (2000/5507: k_upfirdn_rows_direct)."""
    from offline_tarteel_amd.audio import load_audio, load_audio_device, probe_samples

    rng = np.random.default_rng(44)
    specs = [(44100, 2, "pcm16", 30011), (16000, 1, "pcm16", 9000), (48000, 1, "f32", 24001), (22050, 3, "f32", 5000),
             (44100, 2, "pcm16", 1234), (16000, 2, "f32", 4000),
             (48000, 8, "f32", 12001), (44100, 2, "pcm24", 7001), (11025, 1, "u8", 6000), (22050, 1, "f64", 5001),
             (44100, 2, "ext_pcm16", 3003), (44056, 1, "f32", 9000)]
    paths = []
    for k, (sr, ch, kind, n) in enumerate(specs):
        p = tmp_path / f"c{k}.wav"
        _wav(p, (rng.standard_normal(n * ch) * 0.2).astype(np.float32), sr, ch, kind)
        paths.append(str(p))
    dev, lens = load_audio_device(paths, eng)
    dev = dev.cpu().numpy()
    assert dev.shape == (len(paths), max(lens))
    for k, p in enumerate(paths):
        want = load_audio(p)
        assert lens[k] == len(want), (k, lens[k], len(want))
        assert np.array_equal(dev[k, : lens[k]].view(np.uint32), want.view(np.uint32)), specs[k]
        assert not dev[k, lens[k]:].any()
        assert abs(probe_samples(p) - len(want)) <= 1                       # the header probe the sharded runner sorts by


# ---------------------------------------------------------------- every path the ingest kernels take ----
# tests/audio_ref.py names the shapes; tests/test_audio_host.py holds the numpy restatements of the kernels to scipy / numpy
# at every one of them on the CPU and shows that a left-to-right channel sum, a fused multiply-add and a flush of subnormals
# each differ from the references on these inputs.

def _lds_bytes(up, down):
    """the 60 KB rule of launch_upfirdn_rows (csrc/qv_ingest.hip), restated: the per-phase filter (up * P taps) and the
    window of x a block of 256 outputs reads (256 * down / up + P + 2 samples), as float32"""
    from offline_tarteel_amd.audio import resample_plan

    n_taps = len(resample_plan(up, down, 1)[2])
    P = (n_taps + up - 1) // up
    return (up * P + (256 * down) // up + P + 2) * 4


def _takes_lds_kernel(up, down):
    return _lds_bytes(up, down) <= 60 * 1024       # launch_upfirdn_rows: k_upfirdn_rows if so, k_upfirdn_rows_direct if not


def _zero_bits(a):
    return not a.view(np.uint32).any()


def _resample_case(eng, up, down, lens, name="gauss", spare=300):
    """the rows of a case through resample_rows, picked out of a larger matrix in another order than they lie there, into a
    pitch `spare` samples longer than the longest output: every row scipy's bits, exact zeros behind it"""
    from scipy.signal import resample_poly

    import audio_ref as A

    rows = A.case_rows(up, down, lens, name)
    R = len(lens)
    x = np.zeros((R + 2, max(lens) + 13), dtype=np.float32)
    src = [R - k for k in range(R)]                                        # output row k <- source row R - k; rows 0 and R + 1 unused
    for k, row in enumerate(rows):
        x[src[k], : len(row)] = row
    n_want = [(n * up + down - 1) // down for n in lens]
    pitch = max(n_want) + spare
    y, n_out = eng.resample_rows(torch.from_numpy(x).cuda(), lens, up, down, src_rows=src, out_pitch=pitch)
    y = y.cpu().numpy()
    assert y.shape == (R, pitch) and n_out == n_want
    for k, row in enumerate(rows):
        want = resample_poly(row, up, down)
        assert len(want) == n_out[k]
        assert np.array_equal(y[k, : n_out[k]].view(np.uint32), want.view(np.uint32)), (up, down, lens[k], name)
        assert _zero_bits(y[k, n_out[k]:]), (up, down, lens[k], name)
    return y, n_out


def _cases(table):
    import audio_ref as A

    return [(up, down, lens) for (up, down), lens in getattr(A, table).items()]


@pytest.mark.parametrize("up,down,lens", _cases("DIRECT_CASES"))
def test_direct_kernel_equals_scipy(eng, up, down, lens):
    """k_upfirdn_rows_direct, the kernel of every ratio whose filter and window exceed 60 KB of LDS"""
    assert not _takes_lds_kernel(up, down), _lds_bytes(up, down)
    n_out = [(n * up + down - 1) // down for n in lens]
    assert 257 in n_out and min(lens) == 1                                 # one sample past a block of 256; a 1-sample row
    _resample_case(eng, up, down, lens, spare=7)


@pytest.mark.parametrize("up,down,lens", _cases("LDS_LARGEST_CASE"))
def test_lds_kernel_at_its_largest_footprint(eng, up, down, lens):
    """k_upfirdn_rows at 11,025 Hz -> 16 kHz: 54,556 bytes of dynamic LDS, under the launcher's 61,440 by a tenth"""
    assert _takes_lds_kernel(up, down) and _lds_bytes(up, down) == 54556
    n_out = [(n * up + down - 1) // down for n in lens]
    assert 257 in n_out and min(lens) == 1
    _resample_case(eng, up, down, lens, spare=7)


GRID_OUTPUTS = 4096 * 256       # launch_upfirdn_rows / launch_mixdown cap the grid at 4,096 blocks of 256 outputs a row


@pytest.mark.parametrize("up,down,lens", _cases("GRID_STRIDE_CASES"))
def test_lds_kernel_second_grid_pass(eng, up, down, lens):
    """rows of more than 4,096 blocks: k_upfirdn_rows' blocks restage their window of x for a second pass.  (9, 10): one
    output in the second pass (1,165,085 samples), a last block that straddles n_out, a short row whose later blocks lie
    wholly in the padding; (1, 3): a window that moves three input samples per output"""
    assert _takes_lds_kernel(up, down)
    n_out = [(n * up + down - 1) // down for n in lens]
    assert max(n_out) > GRID_OUTPUTS and min(n_out) < 2 * 256
    if (up, down) == (9, 10):
        assert n_out[0] == GRID_OUTPUTS + 1 and n_out[2] == GRID_OUTPUTS
    _resample_case(eng, up, down, lens, spare=300)


@pytest.mark.parametrize("up,down,lens", _cases("GRID_STRIDE_DIRECT_CASE"))
def test_direct_kernel_second_grid_pass(eng, up, down, lens):
    assert not _takes_lds_kernel(up, down)
    assert (max(lens) * up + down - 1) // down > GRID_OUTPUTS
    _resample_case(eng, up, down, lens, spare=300)


def _mixdown_case(eng, channels, frames, name, seed=0):
    """rows of `frames` frames through mixdown_rows: numpy's mean and its restatement bit for bit, exact zeros behind"""
    import audio_ref as A

    x = np.zeros((len(frames), max(frames) * channels), dtype=np.float32)
    for r, n in enumerate(frames):
        x[r, : n * channels] = A.pattern(name, n * channels, seed=seed + r)
    y = eng.mixdown_rows(torch.from_numpy(x).cuda(), frames, channels).cpu().numpy()
    assert y.shape == (len(frames), max(frames))
    for r, n in enumerate(frames):
        want = x[r, : n * channels].reshape(-1, channels).mean(axis=1)
        assert want.dtype == np.float32
        assert np.array_equal(y[r, :n].view(np.uint32), want.view(np.uint32)), (channels, name, r)
        assert np.array_equal(y[r, :n].view(np.uint32), A.mixdown_restatement(x[r, : n * channels], channels).view(np.uint32)), (channels, name, r)
        assert _zero_bits(y[r, n:]), (channels, name, r)


@pytest.mark.parametrize("name", ["gauss", "half_zeros", "neg_zeros"])
@pytest.mark.parametrize("channels", [1, 2, 7, 8, 9, 15, 16, 17, 33, 63, 64])
def test_mixdown_every_channel_count_is_numpy_mean(eng, channels, name):
    """numpy sums 8 channels and more as eight running sums joined by a fixed tree, and gives +0.0 for a frame of -0.0"""
    _mixdown_case(eng, channels, [1000, 1, 777], name, seed=channels)


@pytest.mark.parametrize("channels", [2, 8])
def test_mixdown_second_grid_pass(eng, channels):
    _mixdown_case(eng, channels, [GRID_OUTPUTS + 1, GRID_OUTPUTS + 300, 1], "gauss", seed=channels)


def _edge_cases():
    import audio_ref as A

    return [(up, down, name) for up, down in A.EDGE_RATIOS for name in A.PATTERNS]


@pytest.mark.parametrize("up,down,name", _edge_cases())
def test_fir_numeric_edges(eng, up, down, name):
    """subnormal products and sums, signed zeros, full scale: k_upfirdn and the batched kernel both scipy's bits.  scipy's
    outputs on the "tiny" pattern are subnormal almost throughout: a build that flushed them would fail here."""
    from scipy.signal import resample_poly

    import audio_ref as A

    _resample_case(eng, up, down, A.EDGE_LENGTHS, name, spare=5)
    for row in A.case_rows(up, down, A.EDGE_LENGTHS, name):
        want = resample_poly(row, up, down)
        got = eng.resample_poly(torch.from_numpy(row).cuda(), up, down).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (up, down, len(row), name)


def test_forty_calls_in_flight_share_the_row_table_ring_and_the_filter_cache(eng):
    """40 calls on one stream with no synchronisation between them, each with a row table of its own: the 16-slot ring of
    tables wraps twice and three filters are looked up in turn"""
    from scipy.signal import resample_poly

    import audio_ref as A

    ratios, counts = [(9, 10), (11, 10), (160, 441)], [2, 8]
    plan, inputs = [], []
    for k in range(40):
        if k % 5 < 3:
            lens = [200 + 37 * k, 50 + k, 1 + k % 3]
            rows = A.case_rows(*ratios[k % 5], lens, "gauss")
            x = np.zeros((3, max(lens)), dtype=np.float32)
        else:
            ch = counts[k % 5 - 3]
            lens = [100 + 11 * k, 1 + k % 4, 60 + k]                       # frames
            rows = [A.pattern("gauss", n * ch, seed=k) for n in lens]
            x = np.zeros((3, max(lens) * ch), dtype=np.float32)
        for r, row in enumerate(rows):
            x[r, : len(row)] = row
        plan.append((k % 5, lens, rows))
        inputs.append(torch.from_numpy(x).cuda())
    plan.append(plan[0])
    inputs.append(inputs[0])
    torch.cuda.synchronize()
    outs = []
    for (kind, lens, rows), x in zip(plan, inputs):                       # no synchronisation in here
        outs.append(eng.resample_rows(x, lens, *ratios[kind])[0] if kind < 3 else eng.mixdown_rows(x, lens, counts[kind - 3]))
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    for k, ((kind, lens, rows), y) in enumerate(zip(plan, outs)):
        for r, row in enumerate(rows):
            want = resample_poly(row, *ratios[kind]) if kind < 3 else row.reshape(-1, counts[kind - 3]).mean(axis=1)
            assert np.array_equal(y[r, : len(want)].view(np.uint32), want.view(np.uint32)), (k, kind, r)
            assert _zero_bits(y[r, len(want):]), (k, kind, r)
    assert np.array_equal(outs[0].view(np.uint32), outs[-1].view(np.uint32))


def test_more_rows_than_one_call_takes(eng):
    """1,030 rows: Engine.resample_rows / mixdown_rows split them into calls of at most 1,024 (QV_RESAMPLE_ROWS) that write
    into one output"""
    from scipy.signal import resample_poly

    import audio_ref as A

    R, up, down = 1030, 9, 10
    assert R > eng.RESAMPLE_ROWS
    lens = [5 + (7 * r) % 36 for r in range(R)]
    assert min(lens) == 5 and max(lens) == 40
    rows = [A.pattern("gauss", n, seed=r) for r, n in enumerate(lens)]
    x = np.zeros((R, 43), dtype=np.float32)
    for r, row in enumerate(rows):
        x[r, : len(row)] = row
    want = [resample_poly(row, up, down) for row in rows]
    src = [(r * 7) % R for r in range(R)]                                  # a permutation: 7 and 1,030 are coprime
    assert sorted(src) == list(range(R))
    d = torch.from_numpy(x).cuda()
    y0, n0 = eng.resample_rows(d, lens, up, down, out_pitch=41)
    y1, n1 = eng.resample_rows(d, [lens[s] for s in src], up, down, src_rows=src)
    y0, y1 = y0.cpu().numpy(), y1.cpu().numpy()
    for r in range(R):
        assert n0[r] == len(want[r]) and n1[r] == len(want[src[r]])
        assert np.array_equal(y0[r, : n0[r]].view(np.uint32), want[r].view(np.uint32)) and _zero_bits(y0[r, n0[r]:]), r
        assert np.array_equal(y1[r, : n1[r]].view(np.uint32), want[src[r]].view(np.uint32)) and _zero_bits(y1[r, n1[r]:]), r
    frames = [n // 2 for n in lens]
    m = eng.mixdown_rows(d, frames, 2).cpu().numpy()
    assert m.shape == (R, 20)
    for r, n in enumerate(frames):
        w = x[r, : 2 * n].reshape(-1, 2).mean(axis=1)
        assert np.array_equal(m[r, :n].view(np.uint32), w.view(np.uint32)) and _zero_bits(m[r, n:]), r
