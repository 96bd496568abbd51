"""The audio ingest on the CPU: the premises of tests/test_gpu_audio.py and the WAV decoder.

The GPU tests compare k_mixdown and the three k_upfirdn* kernels with numpy.mean and scipy.signal.resample_poly bit for bit.
Here the restatements of tests/audio_ref.py are held to the same two references (so "equals numpy / scipy" and "computes
what the header says" are one statement), and the planted errors -- a left-to-right channel sum, a fused multiply-add, a
flush of subnormals -- are shown to differ from them on the very inputs the GPU tests use: a kernel with one of these defects
cannot pass there.  audio._decode_wav is held to samples built from integers by the documented scale."""
import math
import struct

import numpy as np
import pytest
from scipy.signal import resample_poly

import audio_ref as A
from offline_tarteel_amd.audio import _decode_wav, load_audio, probe_samples, resample_plan

FRAMES = 300


def _numpy_mean(x, ch):
    return x.reshape(-1, ch).mean(axis=1)


# ---------------------------------------------------------------- mix-down ----
@pytest.mark.parametrize("name", A.PATTERNS)
def test_mixdown_restatement_is_numpy_mean(name):
    for ch in range(1, 65):
        x = A.pattern(name, FRAMES * ch, seed=ch)
        want = _numpy_mean(x, ch)
        assert want.dtype == np.float32
        assert np.array_equal(A.bits(A.mixdown_restatement(x, ch)), A.bits(want)), (name, ch)


def test_sequential_sum_is_not_numpy_mean_from_8_channels():
    """the power of the GPU's channel-count cases against a left-to-right sum: at least a tenth of the frames differ"""
    for ch in range(1, 65):
        x = A.pattern("gauss", 5000 * ch, seed=ch)
        differ = int((A.bits(A.mixdown_sequential(x, ch)) != A.bits(_numpy_mean(x, ch))).sum())
        if ch < 8:
            assert differ == 0, (ch, differ)
        else:
            assert differ >= 500, (ch, differ)


def test_sequential_sum_keeps_the_negative_zero_numpy_drops():
    for ch in range(1, 65):
        x = A.pattern("neg_zeros", FRAMES * ch)
        want = _numpy_mean(x, ch)
        assert not np.signbit(want).any(), ch                       # numpy: +0.0 at every count
        if ch >= 2:
            assert np.signbit(A.mixdown_sequential(x, ch)).all(), ch


# ---------------------------------------------------------------- polyphase FIR ----
def _resampler_shapes():
    out = []
    for cases in (A.DIRECT_CASES, A.LDS_LARGEST_CASE, A.GRID_STRIDE_CASES, A.GRID_STRIDE_DIRECT_CASE):
        out += [(up, down, tuple(lens), "gauss") for (up, down), lens in cases.items()]
    for up, down in A.EDGE_RATIOS:
        out += [(up, down, tuple(A.EDGE_LENGTHS), name) for name in A.PATTERNS]
    return out


@pytest.mark.parametrize("up,down,lens,name", _resampler_shapes())
def test_upfirdn_restatement_is_scipy_at_every_gpu_shape(up, down, lens, name):
    for n, x in zip(lens, A.case_rows(up, down, lens, name)):
        u, d, taps, m0, n_out = resample_plan(up, down, n)
        want = resample_poly(x, up, down)
        assert want.dtype == np.float32 and len(want) == n_out
        got = A.upfirdn_restatement(x, taps, u, d, m0, n_out)
        assert np.array_equal(A.bits(got), A.bits(want)), (up, down, n, name)


@pytest.mark.parametrize("up,down", A.EDGE_RATIOS)
def test_planted_fir_errors_differ_from_scipy(up, down):
    tiny = np.finfo(np.float32).tiny
    for n, xg, xt in zip(A.EDGE_LENGTHS, A.case_rows(up, down, A.EDGE_LENGTHS, "gauss"), A.case_rows(up, down, A.EDGE_LENGTHS, "tiny")):
        u, d, taps, m0, n_out = resample_plan(up, down, n)
        want = resample_poly(xt, up, down)
        assert int(((want != 0) & (np.abs(want) < tiny)).sum()) >= n_out // 4, (up, down, n)     # scipy keeps subnormals
        assert not np.array_equal(A.bits(A.upfirdn_flushed(xt, taps, u, d, m0, n_out)), A.bits(want)), (up, down, n)
        assert not np.array_equal(A.bits(A.upfirdn_fused(xg, taps, u, d, m0, n_out)), A.bits(resample_poly(xg, up, down))), (up, down, n)


def test_every_length_asks_for_the_same_filter_padding():
    """Engine.resample_rows hands one filter to a whole batch: the longest zero-padded one any row's length asks for.  No two
    lengths ask for different ones: resample_plan's padding in front depends on the ratio alone, and the padding behind
    depends on the length only through n * up mod down, so lengths 1 ... down cover a ratio completely.  Searched: every
    coprime (up, down) with both in 1 ... 24, and (160, 441), (320, 441), (640, 441), (147, 160), (441, 160), (1, 3),
    (800, 801), (801, 800), (2000, 5507), each at every length 1 ... 2 * down + 1 -- one tap count per ratio throughout.  The
    max() in resample_rows is therefore unexercised by any input found, and no GPU case can be built for it."""
    ratios = [(u, d) for u in range(1, 25) for d in range(1, 25) if math.gcd(u, d) == 1 and (u, d) != (1, 1)]
    ratios += [(160, 441), (320, 441), (640, 441), (147, 160), (441, 160), (800, 801), (801, 800), (2000, 5507)]
    for up, down in ratios:
        counts = {len(resample_plan(up, down, n)[2]) for n in range(1, 2 * down + 2)}
        assert len(counts) == 1, (up, down, counts)


# ---------------------------------------------------------------- WAV decoding ----
EDGE24 = [-0x800000, 0x7FFFFF, -1, 1]          # the bit patterns 0x800000, 0x7FFFFF, 0xFFFFFF, 0x000001
ENCODINGS = ["u8", "pcm16", "pcm24", "pcm32", "f32", "f64", "ext_pcm16", "ext_pcm24", "ext_f32"]


def _encode(kind, n, seed):
    """(payload bytes, tag, bits, extensible, expected float32 samples) of n samples"""
    rng = np.random.default_rng(seed)
    ext, kind = kind.startswith("ext_"), kind.replace("ext_", "")
    if kind in ("f32", "f64"):
        x = (rng.standard_normal(n) * 0.3).astype(np.float64 if kind == "f64" else np.float32)
        return x.astype("<f8" if kind == "f64" else "<f4").tobytes(), 3, x.itemsize * 8, ext, x.astype(np.float32)
    b = {"u8": 8, "pcm16": 16, "pcm24": 24, "pcm32": 32}[kind]
    v = rng.integers(0, 256, n) if b == 8 else rng.integers(-(1 << (b - 1)), 1 << (b - 1), n)
    if b == 8:
        v[:2] = [0, 255]
    else:
        edge = [-(1 << (b - 1)), (1 << (b - 1)) - 1, -1, 1]
        v[: min(4, n)] = edge[: min(4, n)]
    return A.pcm_bytes(v, b), 1, b, ext, A.pcm_scale(v, b)


def test_24_bit_edge_patterns_are_what_the_encoder_writes():
    assert A.pcm_bytes(EDGE24, 24) == bytes.fromhex("000080" "ffff7f" "ffffff" "010000")
    assert A.pcm_scale(EDGE24, 24).tolist() == [-1.0, 8388607 / 8388608, -1 / 8388608, 1 / 8388608]


@pytest.mark.parametrize("kind", ENCODINGS)
@pytest.mark.parametrize("channels", [1, 2, 8])
def test_decode_wav_every_encoding(tmp_path, kind, channels):
    frames, sr = 203, 22050
    payload, tag, b, ext, want = _encode(kind, frames * channels, seed=channels)
    p = tmp_path / "a.wav"
    p.write_bytes(A.wav_bytes(payload, sr, channels, tag, b, extensible=ext))
    x, ch, rate = _decode_wav(p)
    assert (ch, rate) == (channels, sr) and x.dtype == np.float32
    assert np.array_equal(A.bits(x), A.bits(want))
    mono = want.reshape(-1, channels).mean(axis=1).astype(np.float32) if channels > 1 else want
    got = load_audio(str(p))
    assert np.array_equal(A.bits(got), A.bits(resample_poly(mono, 320, 441).astype(np.float32)))
    assert abs(probe_samples(str(p)) - len(got)) <= 1


@pytest.mark.parametrize("kind", ["pcm16", "pcm24", "u8", "f32"])
def test_decode_wav_odd_chunk_and_partial_frame(tmp_path, kind):
    """a LIST chunk of odd size (its pad byte must be skipped to find ``data``) and a data chunk that ends inside a frame"""
    channels, frames = 2, 101
    payload, tag, b, ext, want = _encode(kind, frames * channels, seed=9)
    p = tmp_path / "a.wav"
    p.write_bytes(A.wav_bytes(payload, 16000, channels, tag, b, before_data=A.odd_list_chunk()))
    x, ch, rate = _decode_wav(p)
    assert (ch, rate) == (2, 16000) and np.array_equal(A.bits(x), A.bits(want))
    # one sample more than whole frames; for 24 bits also a byte, and a sample and a byte, more than whole samples
    for extra in [b // 8] + ([1, 4] if kind == "pcm24" else []):
        p.write_bytes(A.wav_bytes(payload + payload[:extra], 16000, channels, tag, b, before_data=A.odd_list_chunk()))
        x, ch, rate = _decode_wav(p)
        assert len(x) == frames * channels and np.array_equal(A.bits(x), A.bits(want)), (kind, extra)
        assert probe_samples(str(p)) == frames


def test_decode_wav_refusals(tmp_path):
    p = tmp_path / "a.wav"
    pcm = A.pcm_bytes(np.arange(40), 16)
    for tag, b in ((2, 4), (6, 8), (7, 8), (1, 12), (3, 16), (85, 16)):              # ADPCM, A-law, mu-law, 12-bit, half, mp3
        p.write_bytes(A.wav_bytes(pcm, 16000, 1, tag, b if b % 8 == 0 else 16))
        if b % 8:
            raw = bytearray(p.read_bytes())
            raw[34:36] = struct.pack("<H", b)
            p.write_bytes(bytes(raw))
        with pytest.raises(ValueError, match="unsupported WAV encoding"):
            _decode_wav(p)
    p.write_bytes(A.wav_bytes(pcm, 16000, 1, 0x11, 16, extensible=True))             # EXTENSIBLE around an unsupported sub-format
    with pytest.raises(ValueError, match="unsupported WAV encoding"):
        _decode_wav(p)
    whole = A.wav_bytes(pcm, 16000, 1, 1, 16)
    no_fmt = whole[:12] + whole[12 + 24:]
    no_data = whole[: 12 + 24]
    for raw in (no_fmt, no_data):
        p.write_bytes(raw[:4] + struct.pack("<I", len(raw) - 8) + raw[8:])
        with pytest.raises(ValueError, match="malformed WAV"):
            _decode_wav(p)
    p.write_bytes(b"ID3\x00" * 8)
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        _decode_wav(p)
