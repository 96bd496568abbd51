"""Plain-numpy restatements of the ingest kernels (k_mixdown, k_upfirdn, k_upfirdn_rows, k_upfirdn_rows_direct), planted
errors of each, the seeded input patterns the audio tests share and a WAV writer for every encoding audio._decode_wav reads.
No HIP: tests/test_audio_host.py holds every restatement to numpy / scipy on the CPU and shows that every plant differs from
them; tests/test_gpu_audio.py holds the kernels to numpy / scipy (and to the restatements) on the device."""
import struct

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------- mix-down ----
def mixdown_restatement(x, channels):
    """x.reshape(-1, channels).mean(axis=1) of interleaved float32 samples, restated: numpy's float32 add-reduce along a
    contiguous axis (the pairwise-sum inner loop of its add ufunc) for 1 ... 128 elements, then one division by the count.

    Below 8 elements numpy adds them left to right onto 0.  From 8 elements up it keeps eight running sums, r[k] = a[k] and
    r[k] += a[i + k] for i = 8, 16, ... over the whole groups of eight, joins them as
    ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and adds the n % 8 tail elements one by one.  The reduction's result
    starts from the identity +0, so a frame whose channels are all -0.0 sums to +0.0 in both cases."""
    f = np.ascontiguousarray(x, dtype=F32).reshape(-1, channels)
    if channels < 8:
        acc = np.zeros(len(f), F32)
        for c in range(channels):
            acc = acc + f[:, c]
    else:
        r = [f[:, k].copy() for k in range(8)]
        c = 8
        while c + 8 <= channels:
            for k in range(8):
                r[k] = r[k] + f[:, c + k]
            c += 8
        acc = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for t in range(c, channels):
            acc = acc + f[:, t]
        acc = acc + F32(0.0)
    assert acc.dtype == F32
    return acc / F32(channels)


def mixdown_sequential(x, channels):
    """planted error: the channels summed left to right starting from the first one, whatever their number"""
    f = np.ascontiguousarray(x, dtype=F32).reshape(-1, channels)
    acc = f[:, 0].copy()
    for c in range(1, channels):
        acc = acc + f[:, c]
    return acc / F32(channels)


# ---------------------------------------------------------------- polyphase FIR ----
def _step_plain(acc, xs, hs):
    return acc + (xs * hs).astype(F32)


def _step_fused(acc, xs, hs):
    return (acc.astype(np.float64) + xs.astype(np.float64) * hs.astype(np.float64)).astype(F32)   # one rounding per step


_TINY = np.finfo(F32).tiny


def _flush(v):
    return np.where(np.abs(v) < _TINY, F32(0.0), v).astype(F32)


def _step_flushed(acc, xs, hs):
    return _flush(acc + _flush((xs * hs).astype(F32)))


def _upfirdn(x, taps, up, down, m0, n_out, step):
    x = np.ascontiguousarray(x, dtype=F32)
    P = (len(taps) + up - 1) // up
    hp = np.zeros(up * P, F32)
    hp[: len(taps)] = taps
    m = np.arange(m0, m0 + n_out, dtype=np.int64)
    xi, t = (m * down) // up, (m * down) % up
    acc = np.zeros(n_out, F32)
    with np.errstate(under="ignore"):
        for j in range(P):
            i = xi - (P - 1) + j
            ok = (i >= 0) & (i < len(x))
            acc = np.where(ok, step(acc, x[np.clip(i, 0, len(x) - 1)], hp[t + up * (P - 1 - j)]), acc)
    assert acc.dtype == F32
    return acc


def upfirdn_restatement(x, taps, up, down, m0, n_out):
    """numpy restatement of k_upfirdn's arithmetic (include/qverse.h: qv_upfirdn): per output
    sample, products accumulated in float32 in ascending input order."""
    return _upfirdn(x, taps, up, down, m0, n_out, _step_plain)


def upfirdn_fused(x, taps, up, down, m0, n_out):
    """planted error: every step one fused multiply-add, float32(float64(acc) + float64(x) * float64(h))"""
    return _upfirdn(x, taps, up, down, m0, n_out, _step_fused)


def upfirdn_flushed(x, taps, up, down, m0, n_out):
    """planted error: subnormal products and partial sums set to zero, as a build that flushed float32 denormals would"""
    return _upfirdn(x, taps, up, down, m0, n_out, _step_flushed)


# ---------------------------------------------------------------- input patterns ----
PATTERNS = ("gauss", "tiny", "const_denorm", "half_zeros", "neg_zeros", "square")


def pattern(name, n, seed=0):
    """n float32 samples of a named pattern, the same for the same (name, n, seed)"""
    rng = np.random.default_rng([PATTERNS.index(name), int(n), int(seed)])
    if name == "gauss":
        return (rng.standard_normal(n) * 0.3).astype(F32)
    if name == "tiny":                                   # around and below the smallest normal float32: subnormal outputs
        return (rng.standard_normal(n) * 1e-38).astype(F32)
    if name == "const_denorm":                           # the smallest subnormal, negative
        return np.full(n, -1e-45, F32)
    if name == "half_zeros":                             # half of the samples zero, a fifth of those zeros negative
        x = (rng.standard_normal(n) * 0.3).astype(F32)
        z = rng.random(n) < 0.5
        x[z] = F32(0.0)
        x[z & (rng.random(n) < 0.2)] = F32(-0.0)
        return x
    if name == "neg_zeros":
        return np.full(n, -0.0, F32)
    if name == "square":                                 # full scale, +1 / -1
        period = int(rng.integers(2, 40))
        return np.where((np.arange(n) // period) % 2 == 0, F32(1.0), F32(-1.0)).astype(F32)
    raise KeyError(name)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# The resampler shapes of tests/test_gpu_audio.py, (up, down) -> row lengths in samples.  tests/test_audio_host.py holds
# upfirdn_restatement to scipy at every one of them, so a kernel that matches scipy there matches the restatement too.
# Every ratio has a 1-sample row (or the shortest the case allows) and a row of 257 outputs, one past a block of 256.
DIRECT_CASES = {(800, 801): [5000, 4999, 801, 257, 1], (801, 800): [4000, 256, 2, 1], (2000, 5507): [30000, 5507, 706, 1]}
LDS_LARGEST_CASE = {(640, 441): [11025, 177, 3, 1]}
# rows of more than 4,096 blocks x 256 outputs: 1,165,085 samples at 9/10 are 1,048,577 outputs, one in the second pass
GRID_STRIDE_CASES = {(9, 10): [1165085, 1200000, 1165084, 300], (1, 3): [3145734, 7]}
GRID_STRIDE_DIRECT_CASE = {(800, 801): [1050000, 100]}
EDGE_RATIOS = [(9, 10), (11, 10), (160, 441), (1, 3), (800, 801)]
EDGE_LENGTHS = [1000, 257]


def case_rows(up, down, lens, name="gauss"):
    """the rows of a case above: one seeded pattern per length"""
    return [pattern(name, n, seed=up * 100000 + down) for n in lens]


# ---------------------------------------------------------------- WAV files ----
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # bytes 2..15 of KSDATAFORMAT_SUBTYPE_*


def pcm_bytes(values, bits_per_sample):
    """integers -> the little-endian PCM of a WAV file: 8 bits unsigned, 16 / 24 / 32 bits signed two's complement"""
    v = np.asarray(values, dtype=np.int64)
    if bits_per_sample == 8:
        return v.astype(np.uint8).tobytes()
    if bits_per_sample == 24:
        u = (v & 0xFFFFFF).astype("<u4")
        return u.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    return v.astype({16: "<i2", 32: "<i4"}[bits_per_sample]).tobytes()


def wav_bytes(payload, sr, channels, tag, bits_per_sample, extensible=False, before_data=b"", after_data=b""):
    """a RIFF/WAVE file around ``payload``: a 16-byte fmt chunk, or the 40-byte WAVE_FORMAT_EXTENSIBLE one whose sub-format
    carries ``tag``; ``before_data`` are whole chunks (pad byte included) put in front of the data chunk"""
    align = channels * bits_per_sample // 8
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, sr, sr * align, align, bits_per_sample, 22, bits_per_sample,
                          (1 << channels) - 1) + struct.pack("<H", tag) + _KSDATAFORMAT_TAIL
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, sr, sr * align, align, bits_per_sample)
    assert len(fmt) in (16, 40)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + before_data + b"data" + struct.pack("<I", len(payload)) + payload
    body += (b"\0" if len(payload) & 1 else b"") + after_data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def odd_list_chunk():
    """a LIST chunk of odd size followed by its pad byte"""
    text = b"INFOISFT\x05\x00\x00\x00qvrs\x00"
    assert len(text) % 2 == 1
    return b"LIST" + struct.pack("<I", len(text)) + text + b"\0"


def quantise(x, bits_per_sample):
    """float samples in [-1, 1) -> the integers of a PCM file of that width (8 bits: unsigned, offset 128)"""
    if bits_per_sample == 8:
        return np.clip(np.round(np.asarray(x, np.float64) * 128.0) + 128, 0, 255).astype(np.int64)
    full = float(1 << (bits_per_sample - 1))
    return np.clip(np.round(np.asarray(x, np.float64) * full), -full, full - 1).astype(np.int64)


def pcm_scale(values, bits_per_sample):
    """the documented scale of integer PCM: (u - 128) / 128 for 8 bits, v / 2^(bits - 1) otherwise -- exact in float64 (a
    division by a power of two), rounded once to float32"""
    v = np.asarray(values, dtype=np.int64).astype(np.float64)
    if bits_per_sample == 8:
        return ((v - 128.0) / 128.0).astype(F32)
    return (v / float(1 << (bits_per_sample - 1))).astype(F32)
