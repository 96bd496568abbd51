"""ctypes binding of libqverse.so (include/qverse.h) + the host-side glue the plugin needs.

PyTorch-ROCm is used for device memory and streams only: tensors are handed to the C ABI as
raw device pointers.  There is NO CPU fallback: if the HIP library is missing or no GPU is
visible, construction raises.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import LIB_PATH, TABLES_PATH
from .normalizer import normalize_arabic
from .tables import Tables

QV_SOURCE = {0: None, 1: "text", 2: "ctc"}
QV_MAX_TRANSCRIPT = 1024   # include/qverse.h: characters the device matchers hold per text (the default window)
QV_MAX_TRANSCRIPT_WIDE = 2048   # ... and with Engine(max_transcript=2048)


def front_window(text: str, limit: int = QV_MAX_TRANSCRIPT) -> str:
    """The longest whole-word prefix of `text` that fits the device's matching window.  The reference's
    single-text matchers (QuranDB.match_verse behind run_on_full_transcript, VerseTracker._find_best_match)
    take texts of any length; both match -- and then peel -- the FRONT of the text, so a longer text is
    matched on its first `limit` characters instead of being refused (documented difference)."""
    if len(text) <= limit:
        return text
    cut = text.rfind(" ", 0, limit + 1)
    return text[:cut] if cut > 0 else text[:limit]
FLAG_EMPTY, FLAG_TRUNC, FLAG_USED_CTC, FLAG_CAND_OVERFLOW = 1, 2, 4, 8


class QvError(RuntimeError):
    pass


def _p(a):
    """a numpy array as the pointer the C ABI takes; None is a null pointer"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class QvConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32),
        ("tables_path", C.c_char_p), ("weights_path", C.c_char_p),
        ("random_weights_seed", C.c_uint64),
        ("with_model", C.c_int32), ("precision", C.c_int32),
        ("max_batch", C.c_int32), ("max_samples", C.c_int32),
        ("top_text", C.c_int32), ("top_span_refs", C.c_int32), ("max_span", C.c_int32),
        ("threshold", C.c_double), ("text_weight", C.c_double), ("span_penalty", C.c_double),
        ("skip_unused_passes", C.c_int32), ("n_contexts", C.c_int32),
        ("max_transcript", C.c_int32),
    ]


class QvResult(C.Structure):
    _fields_ = [
        ("surah", C.c_int32), ("ayah", C.c_int32), ("ayah_end", C.c_int32), ("source", C.c_int32),
        ("score", C.c_double), ("base_score", C.c_double), ("ctc_norm_loss", C.c_float),
        ("n_tokens", C.c_int32), ("n_chars", C.c_int32), ("n_candidates", C.c_int32),
        ("flags", C.c_int32), ("t_frames", C.c_int32),
    ]


class QvTrackMatch(C.Structure):
    """include/qverse.h: qv_track_match"""
    _fields_ = [("verse", C.c_int32), ("surah", C.c_int32), ("ayah", C.c_int32), ("variant", C.c_int32),
                ("n_words", C.c_int32), ("reserved", C.c_int32), ("score", C.c_double)]


class QvAlignInfo(C.Structure):
    """include/qverse.h: qv_align_info"""
    _fields_ = [("n_tokens", C.c_int32), ("flags", C.c_int32), ("t_frames", C.c_int32), ("start_verse", C.c_int32),
                ("span", C.c_int32), ("reserved", C.c_int32), ("score", C.c_float), ("reserved_f", C.c_float)]


ALIGN_MAX_TOKENS = 383   # include/qverse.h: QV_ALIGN_MAX_TOKENS
ALIGN_NO_TARGET, ALIGN_TOO_LONG, ALIGN_INFEASIBLE = 1, 2, 4
ALIGN_INFO_DTYPE = np.dtype([("n_tokens", "<i4"), ("flags", "<i4"), ("t_frames", "<i4"), ("start_verse", "<i4"),
                             ("span", "<i4"), ("reserved", "<i4"), ("score", "<f4"), ("reserved_f", "<f4")])
assert ALIGN_INFO_DTYPE.itemsize == C.sizeof(QvAlignInfo)

NBEST_MAX = 32           # include/qverse.h: QV_NBEST_MAX
NBEST_TEXT_RUNNERS = 1   # QV_NBEST_TEXT_RUNNERS


class QvNbestEntry(C.Structure):
    """include/qverse.h: qv_nbest_entry"""
    _fields_ = [("surah", C.c_int32), ("ayah", C.c_int32), ("ayah_end", C.c_int32), ("start_verse", C.c_int32),
                ("span", C.c_int32), ("cand_index", C.c_int32), ("source", C.c_int32), ("n_tokens", C.c_int32),
                ("score", C.c_double), ("text_score", C.c_double), ("ctc_loss", C.c_float), ("ctc_norm_loss", C.c_float)]


class QvNbestInfo(C.Structure):
    """include/qverse.h: qv_nbest_info"""
    _fields_ = [("n_entries", C.c_int32), ("n_ranked", C.c_int32), ("source", C.c_int32), ("flags", C.c_int32)]


NBEST_ENTRY_DTYPE = np.dtype([("surah", "<i4"), ("ayah", "<i4"), ("ayah_end", "<i4"), ("start_verse", "<i4"), ("span", "<i4"),
                              ("cand_index", "<i4"), ("source", "<i4"), ("n_tokens", "<i4"), ("score", "<f8"),
                              ("text_score", "<f8"), ("ctc_loss", "<f4"), ("ctc_norm_loss", "<f4")], align=True)
NBEST_INFO_DTYPE = np.dtype([("n_entries", "<i4"), ("n_ranked", "<i4"), ("source", "<i4"), ("flags", "<i4")])
assert NBEST_ENTRY_DTYPE.itemsize == C.sizeof(QvNbestEntry) == 56 and NBEST_INFO_DTYPE.itemsize == C.sizeof(QvNbestInfo) == 16

CORRECT_MAX_REF, CORRECT_MAX_WORDS, CORRECT_MAX_RAW = 1280, 288, 2048   # include/qverse.h: QV_CORRECT_MAX_*
CORRECT_PREFIX = 1                                                       # QV_CORRECT_PREFIX (call flag)
CORRECT_NO_TARGET, CORRECT_NO_TRANSCRIPT, CORRECT_TOO_LONG, CORRECT_LAST_WORD_OPEN = 1, 2, 4, 8   # row flags
CORRECT_INFO_FIELDS = ("n_ref", "n_pred", "n_words", "n_ref_used", "words_touched", "distance", "n_match", "n_sub", "n_del",
                       "n_ins", "n_ops", "flags", "start_verse", "span")
CORRECT_WORD_FIELDS = ("n_symbols", "n_match", "n_sub", "n_del", "n_ins", "type")


class QvCorrectInfo(C.Structure):
    """include/qverse.h: qv_correct_info"""
    _fields_ = [(k, C.c_int32) for k in CORRECT_INFO_FIELDS] + [("reserved", C.c_int32 * 2)]


class QvCorrectWord(C.Structure):
    """include/qverse.h: qv_correct_word"""
    _fields_ = [(k, C.c_uint16) for k in CORRECT_WORD_FIELDS]


CORRECT_INFO_DTYPE = np.dtype([(k, "<i4") for k in CORRECT_INFO_FIELDS] + [("reserved", "<i4", (2,))])
CORRECT_WORD_DTYPE = np.dtype([(k, "<u2") for k in CORRECT_WORD_FIELDS])
assert CORRECT_INFO_DTYPE.itemsize == C.sizeof(QvCorrectInfo) == 64 and CORRECT_WORD_DTYPE.itemsize == C.sizeof(QvCorrectWord) == 12


class QvTranscriptInfo(C.Structure):
    """include/qverse.h: qv_transcript_info"""
    _fields_ = [("n_tokens", C.c_int32), ("t_frames", C.c_int32), ("n_blank_frames", C.c_int32), ("flags", C.c_int32),
                ("min_token_logprob", C.c_float), ("reserved_f", C.c_float),
                ("avg_logprob", C.c_double), ("frame_avg_logprob", C.c_double)]


TRANSCRIPT_INFO_DTYPE = np.dtype([("n_tokens", "<i4"), ("t_frames", "<i4"), ("n_blank_frames", "<i4"), ("flags", "<i4"),
                                  ("min_token_logprob", "<f4"), ("reserved_f", "<f4"),
                                  ("avg_logprob", "<f8"), ("frame_avg_logprob", "<f8")])
assert TRANSCRIPT_INFO_DTYPE.itemsize == C.sizeof(QvTranscriptInfo) == 40

class QvLongInfo(C.Structure):
    """include/qverse.h: qv_long_info"""
    _fields_ = [("n_tokens", C.c_int32), ("t_frames", C.c_int32), ("n_blank_frames", C.c_int32), ("flags", C.c_int32),
                ("n_windows", C.c_int32), ("reserved", C.c_int32),
                ("min_token_logprob", C.c_float), ("reserved_f", C.c_float),
                ("avg_logprob", C.c_double), ("frame_avg_logprob", C.c_double)]


LONG_INFO_DTYPE = np.dtype([("n_tokens", "<i4"), ("t_frames", "<i4"), ("n_blank_frames", "<i4"), ("flags", "<i4"),
                            ("n_windows", "<i4"), ("reserved", "<i4"), ("min_token_logprob", "<f4"), ("reserved_f", "<f4"),
                            ("avg_logprob", "<f8"), ("frame_avg_logprob", "<f8")])
assert LONG_INFO_DTYPE.itemsize == C.sizeof(QvLongInfo) == 48
QV_LONG_MAX_FRAMES = 262144
QV_LONG_HOP = 1280   # samples per encoder frame


class QvAlignLongInfo(C.Structure):
    """include/qverse.h: qv_align_long_info"""
    _fields_ = [("n_tokens", C.c_int32), ("flags", C.c_int32), ("t_frames", C.c_int32), ("n_windows", C.c_int32),
                ("score", C.c_float), ("reserved_f", C.c_float)]


ALIGN_LONG_MAX_TOKENS = 16383     # include/qverse.h: QV_ALIGN_LONG_MAX_TOKENS
ALIGN_LONG_MAX_BYTES = 1 << 32    # QV_ALIGN_LONG_MAX_BYTES
ALIGN_LONG_INFO_DTYPE = np.dtype([("n_tokens", "<i4"), ("flags", "<i4"), ("t_frames", "<i4"), ("n_windows", "<i4"),
                                  ("score", "<f4"), ("reserved_f", "<f4")])
assert ALIGN_LONG_INFO_DTYPE.itemsize == C.sizeof(QvAlignLongInfo) == 24

BEAM_MAX = 64        # include/qverse.h: QV_BEAM_MAX
BEAM_COMPLETE = 1    # QV_BEAM_COMPLETE


class QvBeamEntry(C.Structure):
    """include/qverse.h: qv_beam_entry"""
    _fields_ = [("node", C.c_int32), ("n_tokens", C.c_int32), ("n_ends", C.c_int32), ("start_verse", C.c_int32), ("span", C.c_int32),
                ("surah", C.c_int32), ("ayah", C.c_int32), ("ayah_end", C.c_int32), ("below_count", C.c_int32),
                ("below_verse", C.c_int32), ("below_span", C.c_int32), ("flags", C.c_int32),
                ("score", C.c_double), ("blank_score", C.c_double), ("nonblank_score", C.c_double)]


BEAM_ENTRY_DTYPE = np.dtype([("node", "<i4"), ("n_tokens", "<i4"), ("n_ends", "<i4"), ("start_verse", "<i4"), ("span", "<i4"),
                             ("surah", "<i4"), ("ayah", "<i4"), ("ayah_end", "<i4"), ("below_count", "<i4"), ("below_verse", "<i4"),
                             ("below_span", "<i4"), ("flags", "<i4"), ("score", "<f8"), ("blank_score", "<f8"),
                             ("nonblank_score", "<f8")])
BEAM_INFO_DTYPE = np.dtype([("n_entries", "<i4"), ("t_frames", "<i4"), ("max_candidates", "<i4"), ("reserved", "<i4")])
assert BEAM_ENTRY_DTYPE.itemsize == C.sizeof(QvBeamEntry) == 72 and BEAM_INFO_DTYPE.itemsize == 16


def trie_stats(max_span: int = 3, tables_path: str | None = None) -> dict:
    """qv_trie_stats: {"nodes", "ends", "max_depth", "max_children"} of the beam search's trie for max_span in 1..6, from the
    tables file alone -- host only, no engine, no GPU."""
    lib = load_library()
    out = [C.c_int32(0) for _ in range(4)]
    rc = lib.qv_trie_stats(str(tables_path or TABLES_PATH).encode(), int(max_span), *map(C.byref, out))
    if rc != 0:
        msg = lib.qv_last_error(None).decode()
        if rc == 2:
            raise FileNotFoundError(msg)
        raise QvError(f"qv_trie_stats failed ({rc}): {msg}")
    return dict(zip(("nodes", "ends", "max_depth", "max_children"), (int(v.value) for v in out)))


SCAN_MAX = 32        # include/qverse.h: QV_SCAN_MAX


class QvScanEntry(C.Structure):
    """include/qverse.h: qv_scan_entry"""
    _fields_ = [("start_verse", C.c_int32), ("span", C.c_int32), ("surah", C.c_int32), ("ayah", C.c_int32), ("ayah_end", C.c_int32),
                ("n_tokens", C.c_int32), ("loss", C.c_float), ("norm", C.c_float), ("final_score", C.c_double)]


SCAN_ENTRY_DTYPE = np.dtype([("start_verse", "<i4"), ("span", "<i4"), ("surah", "<i4"), ("ayah", "<i4"), ("ayah_end", "<i4"),
                             ("n_tokens", "<i4"), ("loss", "<f4"), ("norm", "<f4"), ("final_score", "<f8")])
SCAN_INFO_DTYPE = np.dtype([("n_entries", "<i4"), ("n_feasible", "<i4"), ("n_recursions", "<i4"), ("t_frames", "<i4")])
assert SCAN_ENTRY_DTYPE.itemsize == C.sizeof(QvScanEntry) == 40 and SCAN_INFO_DTYPE.itemsize == 16


def surah_mask(surahs) -> np.ndarray | None:
    """the 128-bit surah mask of the scan as uint32[4]: bit s - 1 selects surah s; None = every surah"""
    if surahs is None:
        return None
    m = np.zeros(4, np.uint32)
    for s in surahs:
        s = int(s)
        if not 1 <= s <= 128:
            raise ValueError(f"surah {s} outside 1..128")
        m[(s - 1) >> 5] |= np.uint32(1 << ((s - 1) & 31))
    return m


def scan_stats(t_frames: int, max_span: int = 6, surahs=None, tables_path: str | None = None) -> dict:
    """qv_scan_stats: {"n_feasible", "n_recursions", "state_steps"} of the exhaustive CTC scan for a row of t_frames frames,
    from the tables file alone -- host only, no engine, no GPU."""
    lib = load_library()
    nf, nr, ss = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    m = surah_mask(surahs)
    rc = lib.qv_scan_stats(str(tables_path or TABLES_PATH).encode(), int(t_frames), int(max_span),
                           _p(m), C.byref(nf), C.byref(nr), C.byref(ss))
    if rc != 0:
        msg = lib.qv_last_error(None).decode()
        if rc == 2:
            raise FileNotFoundError(msg)
        raise QvError(f"qv_scan_stats failed ({rc}): {msg}")
    return {"n_feasible": int(nf.value), "n_recursions": int(nr.value), "state_steps": int(ss.value)}


RESULT_DTYPE = np.dtype([
    ("surah", "<i4"), ("ayah", "<i4"), ("ayah_end", "<i4"), ("source", "<i4"),
    ("score", "<f8"), ("base_score", "<f8"), ("ctc_norm_loss", "<f4"),
    ("n_tokens", "<i4"), ("n_chars", "<i4"), ("n_candidates", "<i4"),
    ("flags", "<i4"), ("t_frames", "<i4"),
], align=True)
assert RESULT_DTYPE.itemsize == C.sizeof(QvResult)

_lib = None


def load_library(path: Path | str | None = None) -> C.CDLL:
    """Load libqverse.so; fail loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    p = Path(path or os.environ.get("QVERSE_LIB", LIB_PATH))
    if not p.exists():
        raise QvError(f"{p} not found: build it with `python offline-tarteel_amd/build.py` "
                      "(hipcc, gfx950). There is no CPU fallback for this path.")
    lib = C.CDLL(str(p))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.qv_config_default.argtypes = [C.POINTER(QvConfig)]
    lib.qv_config_default.restype = None
    lib.qv_create.argtypes = [C.POINTER(QvConfig), C.POINTER(vp)]
    lib.qv_destroy.argtypes = [vp]
    lib.qv_destroy.restype = None
    lib.qv_last_error.argtypes = [vp]
    lib.qv_last_error.restype = C.c_char_p
    lib.qv_build_info.restype = C.c_char_p
    lib.qv_frames_for_samples.argtypes = [i64]
    lib.qv_frames_for_samples.restype = i32
    lib.qv_forward.argtypes = [vp, vp, vp, i32, i64, vp, i32, vp, vp]
    lib.qv_decode_retrieve_rerank.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.qv_decode_retrieve_rerank_async.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.qv_fetch_results.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.qv_predict_batch.argtypes = [vp, vp, vp, i32, i64, vp, vp, vp]
    lib.qv_predict_batch_async.argtypes = [vp, vp, vp, i32, i64, vp]
    lib.qv_predict_batch_async_ctx.argtypes = [vp, vp, vp, i32, i64, vp, vp]
    lib.qv_packed_results_dev.argtypes = [vp]
    lib.qv_packed_results_dev.restype = vp
    lib.qv_upfirdn.argtypes = [vp, vp, i64, vp, i32, i32, i32, i64, i64, vp, vp]
    lib.qv_upfirdn_batch.argtypes = [vp, vp, i64, vp, vp, i32, vp, i32, i32, i32, i64, vp, i64, vp]
    lib.qv_mixdown_batch.argtypes = [vp, vp, i64, vp, i32, i32, vp, i64, vp]
    lib.qv_context_count.argtypes = [vp]
    lib.qv_max_transcript.argtypes = [vp]
    lib.qv_max_transcript.restype = i32
    lib.qv_probe_concurrent_streams.argtypes = []
    lib.qv_last_context.argtypes = [vp]
    lib.qv_wait_ctx.argtypes = [vp, i32]
    lib.qv_packed_results_ctx.argtypes = [vp, i32, vp]
    lib.qv_packed_results_ctx.restype = vp
    lib.qv_fetch_results_ctx.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.qv_align.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_align_results_ctx.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32]
    lib.qv_nbest_results_ctx.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.qv_nbest_select.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp]
    lib.qv_correct.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp]
    lib.qv_correct_results_ctx.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, i32]
    lib.qv_transcribe.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_transcribe_batch.argtypes = [vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_long_plan.argtypes = [i64, i32, i32, i32, vp, vp, vp, vp]
    lib.qv_transcribe_long.argtypes = [vp, vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_transcribe_windows.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_long_kernel_times.argtypes = [vp, vp]
    lib.qv_align_long_plan.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    lib.qv_align_windows.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_align_long.argtypes = [vp, vp, i64, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.qv_align_long_kernel_times.argtypes = [vp, vp]
    lib.qv_trie_stats.argtypes = [C.c_char_p, i32, vp, vp, vp, vp]
    lib.qv_trie_node_tokens.argtypes = [vp, i32, i32, vp, i32, vp]
    lib.qv_beam_decode.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.qv_beam_batch.argtypes = [vp, vp, vp, i32, i64, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.qv_scan_stats.argtypes = [C.c_char_p, i32, i32, vp, vp, vp, vp]
    lib.qv_scan_logprobs.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, i32, vp, vp, vp, vp, vp]
    lib.qv_scan_batch.argtypes = [vp, vp, vp, i32, i64, i32, C.c_double, i32, vp, vp, vp, vp, vp]
    lib.qv_scan_kernel_times.argtypes = [vp, vp]
    lib.qv_tracker_match.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp]
    lib.qv_match_verse.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp]
    lib.qv_debug_retrieve.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.qv_debug_ctc_loss.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp]
    lib.qv_debug_transcript_codes.argtypes = [vp, i32, i32, vp, i32, vp, vp]
    lib.qv_debug_forward_tap.argtypes = [vp, i32, i32, vp, vp]
    lib.qv_profile_gemm.argtypes = [vp, i32]
    lib.qv_profile_gemm_read.argtypes = [vp, vp, vp, vp]
    lib.qv_profile_replay_gemm.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.qv_profile_replay_kernel.argtypes = [vp, i32, C.c_char_p, i32]
    lib.qv_debug_gemm_tiles.argtypes = [i32]
    lib.qv_debug_gemm_tile_height.argtypes = [i32]
    lib.qv_debug_gemm_pipeline.argtypes = [i32, i32, i32]
    lib.qv_debug_forward_graph_failures.argtypes = [vp]
    lib.qv_debug_forward_graph_failures.restype = i64
    lib.qv_debug_attention_variant.argtypes = [i32]
    lib.qv_debug_kernel_variant.argtypes = [i32, i32]
    lib.qv_debug_forward_graph_stats.argtypes = [vp, vp, vp]
    lib.qv_debug_sub01_plan.argtypes = [i64, i32, vp, vp]
    lib.qv_debug_sub35_plan.argtypes = [i64, i32, vp]
    lib.qv_weights_info.argtypes = [vp, C.c_char_p, i32]
    lib.qv_profile_inject_logprobs.argtypes = [vp, vp, i32, vp, i32]
    lib.qv_profile_stages.argtypes = [vp, i32]
    lib.qv_stage_times.argtypes = [vp, i32, vp]
    _lib = lib
    return lib


def exported_symbols() -> list[str]:
    """Every function include/qverse.h declares (used by the CPU load/export test)."""
    import re

    hdr = (Path(__file__).resolve().parent.parent / "include" / "qverse.h").read_text()
    return sorted(set(re.findall(r"\b(qv_[a-z_0-9]+)\s*\(", hdr)))


def env_knobs() -> dict:
    """CTC_DIRECT_* environment knobs with the reference's names and defaults
    (experiments/c2c-direct/run.py:62-74)."""
    return dict(
        top_text=int(os.getenv("CTC_DIRECT_TOP_TEXT", "100")),
        top_span_refs=int(os.getenv("CTC_DIRECT_TOP_SPAN_REFS", "80")),
        max_span=int(os.getenv("CTC_DIRECT_MAX_SPAN", "6")),
        threshold=float(os.getenv("CTC_DIRECT_THRESHOLD", "0.80")),
        text_weight=float(os.getenv("CTC_DIRECT_TEXT_WEIGHT", "0.0")),
        span_penalty=float(os.getenv("CTC_DIRECT_SPAN_PENALTY", "0.5")),
        stream_gate=stream_gate_default(),   # QVERSE_STREAM_GATE: not a qv_config field (Engine.__init__ takes it out)
    )


_long_env = None


def long_env() -> tuple[float | None, float | None]:
    """(window seconds, margin seconds) from QVERSE_LONG_WINDOW_S / QVERSE_LONG_MARGIN_S, read once; None = the default
    (the largest window the engine accepts; min(50, Kw / 4) frames of margin)"""
    global _long_env
    if _long_env is None:
        def num(name):
            v = os.environ.get(name, "").strip()
            return float(v) if v else None
        _long_env = (num("QVERSE_LONG_WINDOW_S"), num("QVERSE_LONG_MARGIN_S"))
    return _long_env


def stream_gate_default() -> bool:
    """QVERSE_STREAM_GATE=1: the engine-backed streaming row gates its chunks by the engine's own confidence
    (StreamingPipeline.run_on_audio_chunked[_batch], confidence_gate=None).  Off by default."""
    return os.getenv("QVERSE_STREAM_GATE", "0") == "1"


class Engine:
    """One engine per process per GPU (weights + verse tables resident for its lifetime)."""

    def __init__(self, device: int = 0, with_model: bool = True, weights_path: str | None = None,
                 seed: int = 20260630, precision: int = 0, max_batch: int = 64, max_samples: int = 480000,
                 tables_path: str | None = None, skip_unused_passes: bool = True, contexts: int = 1,
                 max_transcript: int = QV_MAX_TRANSCRIPT, **knobs):
        import torch

        if not torch.cuda.is_available():
            raise QvError("no ROCm device visible: the qverse hot path runs on MI355X only (no CPU fallback)")
        self.torch = torch
        self.lib = load_library()
        self.device = device
        self.tables_path = str(tables_path or TABLES_PATH)
        if not Path(self.tables_path).exists():
            raise FileNotFoundError(self.tables_path)
        if weights_path is not None and not Path(weights_path).exists():
            raise FileNotFoundError(f"No weight file at {weights_path}")
        cfg = QvConfig()
        self.lib.qv_config_default(C.byref(cfg))
        cfg.device = device
        self._keep = (self.tables_path.encode(), weights_path.encode() if weights_path else None)
        cfg.tables_path, cfg.weights_path = self._keep
        cfg.random_weights_seed = seed
        cfg.with_model = int(with_model)
        cfg.precision = precision
        cfg.max_batch = max_batch
        cfg.max_samples = max_samples
        cfg.skip_unused_passes = int(skip_unused_passes)
        cfg.n_contexts = int(contexts)
        cfg.max_transcript = int(max_transcript)   # matching window: 1024, or 2048 for the wide kernel set
        self.contexts = int(contexts)
        kn = env_knobs()
        kn.update(knobs)
        kn.pop("stream_gate", None)   # read by the streaming row when it runs, not by the engine
        for k, v in kn.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        with torch.cuda.device(device):
            rc = self.lib.qv_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            msg = self.lib.qv_last_error(None).decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise QvError(f"qv_create failed ({rc}): {msg}")
        self.h = h
        # the engine may run fewer batches in flight than asked for (qv_probe_concurrent_streams, include/qverse.h)
        self.contexts = int(self.lib.qv_context_count(h))
        self.max_transcript = int(self.lib.qv_max_transcript(h))
        self.max_batch = max_batch
        self.max_samples = int(max_samples)
        self.tables = Tables(self.tables_path)

    def close(self):
        if getattr(self, "h", None):
            self.lib.qv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- helpers ----
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise QvError(f"{what} failed ({rc}): {self.lib.qv_last_error(self.h).decode()}")

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def frames_for(self, n_samples: int) -> int:
        return int(self.lib.qv_frames_for_samples(int(n_samples)))

    def _audio_args(self, audio, lengths):
        """(B, N, lengths as int64) of a zero-padded batch: audio a contiguous float32 cuda [B, N], one length per row, none
        above N (the forward reads lengths[b] samples of row b)"""
        assert audio.is_cuda and audio.dtype == self.torch.float32 and audio.is_contiguous() and audio.dim() == 2
        B, N = audio.shape
        ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
        assert len(ln) == B and ln.max() <= N
        return B, N, ln

    def _logprob_args(self, log_probs, t_frames=None, per_row: bool = True):
        """(B, t_max, t_frames as int32 or None) of a contiguous float32 cuda [B, t_max, 1025]; per_row: one count per row"""
        assert log_probs.is_cuda and log_probs.dtype == self.torch.float32 and log_probs.is_contiguous() and log_probs.dim() == 3
        B, t_max, V = log_probs.shape
        assert V == 1025
        if t_frames is None:
            return B, t_max, None
        assert not per_row or len(t_frames) == B
        return B, t_max, np.ascontiguousarray(np.asarray(t_frames, dtype=np.int32))

    def _results(self, res: np.ndarray, greedy: np.ndarray | None) -> list[dict]:
        out = []
        for b in range(len(res)):
            r = res[b]
            d = {
                "surah": int(r["surah"]), "ayah": int(r["ayah"]),
                "ayah_end": int(r["ayah_end"]) if r["surah"] else None,
                "score": float(r["score"]), "source": QV_SOURCE[int(r["source"])],
                "base_score": float(r["base_score"]), "ctc_norm_loss": float(r["ctc_norm_loss"]),
                "n_candidates": int(r["n_candidates"]), "flags": int(r["flags"]),
                "t_frames": int(r["t_frames"]), "use_ctc": bool(r["flags"] & FLAG_USED_CTC),
            }
            if greedy is not None:
                ids = greedy[b, : int(r["n_tokens"])].tolist()
                d["greedy_ids"] = ids
                d["transcript"] = self.transcript_of(ids)
                # the device's own counts of that transcript (greedy tokens, normalised characters): with the text fields,
                # so that a row fetched without them (want_text=False) keeps the numeric fields it always had
                d["n_tokens"], d["n_chars"] = int(r["n_tokens"]), int(r["n_chars"])
            out.append(d)
        return out

    def transcript_of(self, ids) -> str:
        """c2c-direct/run.py:201-204: ids_to_text(...).strip() then normalize_arabic."""
        if not ids:
            return ""
        return normalize_arabic(self.tables.ids_to_text(ids).strip())

    # ---------------------------------------------------------------- stages -----
    def forward(self, audio, lengths):
        """audio: float32 cuda tensor [B, N] (zero padded); lengths: int sequence.
        Returns (log_probs [B, Tmax, 1025] cuda float32, T list)."""
        B, N, ln = self._audio_args(audio, lengths)
        t_max = self.frames_for(int(ln.max()))
        lp = self.torch.empty((B, t_max, 1025), dtype=self.torch.float32, device=audio.device)
        t_out = np.zeros(B, dtype=np.int32)
        rc = self.lib.qv_forward(self.h, C.c_void_p(audio.data_ptr()), _p(ln), B, N, C.c_void_p(lp.data_ptr()), t_max, _p(t_out),
                                 self._stream())
        self._check(rc, "qv_forward")
        return lp, t_out.tolist()

    def decode_retrieve_rerank(self, log_probs, t_frames, want_text: bool = True, align: bool = False,
                               nbest: int | None = None, correct: bool = False, correct_prefix: bool = False) -> list[dict]:
        """align=True: every result dict gains an "alignment" entry (align_results) -- the winner's token ids and the
        frames each of them occupies in `log_probs`.  nbest=K: every dict gains "nbest", the row's list of up to K ranked
        alternatives (nbest_results).  correct=True: every dict gains "correction", the row's word-level comparison of
        the transcript with the winner's text (correct_results with the two texts; correct_prefix=True: in prefix mode)."""
        B, t_max, t = self._logprob_args(log_probs, t_frames, per_row=False)
        res = np.zeros(B, dtype=RESULT_DTYPE)
        greedy = np.full((B, t_max), -1, dtype=np.int32) if want_text else None
        rc = self.lib.qv_decode_retrieve_rerank(self.h, C.c_void_p(log_probs.data_ptr()), _p(t), B, t_max, _p(res), _p(greedy),
                                                self._stream())
        self._check(rc, "qv_decode_retrieve_rerank")
        return self._with_correction(self._with_nbest(self._with_alignment(self._results(res, greedy), align), nbest), correct, correct_prefix)

    def predict_batch(self, audio, lengths, want_text: bool = True, align: bool = False, nbest: int | None = None,
                      correct: bool = False, correct_prefix: bool = False) -> list[dict]:
        B, N, ln = self._audio_args(audio, lengths)
        t_max = self.frames_for(int(ln.max()))
        res = np.zeros(B, dtype=RESULT_DTYPE)
        greedy = np.full((B, t_max), -1, dtype=np.int32) if want_text else None
        rc = self.lib.qv_predict_batch(self.h, C.c_void_p(audio.data_ptr()), _p(ln), B, N, _p(res), _p(greedy), self._stream())
        self._check(rc, "qv_predict_batch")
        return self._with_correction(self._with_nbest(self._with_alignment(self._results(res, greedy), align), nbest), correct, correct_prefix)

    # ---------------------------------------------------------------- recitation correction
    def _with_correction(self, results: list[dict], correct: bool, prefix: bool = False) -> list[dict]:
        if correct:
            for d, c in zip(results, self.correct_results(batch=len(results), prefix=prefix, texts=True)):
                d["correction"] = c
        return results

    def _correct_buffers(self, rows: int):
        ops_pitch = CORRECT_MAX_REF + self.max_transcript
        return (np.zeros(rows, CORRECT_INFO_DTYPE), np.zeros((rows, ops_pitch), np.uint8),
                np.zeros((rows, CORRECT_MAX_WORDS), CORRECT_WORD_DTYPE))

    @staticmethod
    def _corrections(info, ops, words) -> list[dict]:
        out = []
        for b in range(len(info)):
            d = {k: int(info[b][k]) for k in CORRECT_INFO_FIELDS}
            d["ops"] = ops[b, : d["n_ops"]].copy()
            d["words"] = words[b, : d["n_words"]].copy()
            out.append(d)
        return out

    def correct_raw(self, pred_codes, ref_codes, prefix: bool = False):
        """qv_correct on lists of code arrays (alphabet codes with their spaces) as the C ABI's arrays, whole: (info [rows]
        of CORRECT_INFO_DTYPE, ops uint8 [rows, 1280 + window] padded with 0xFF, words [rows, 288] of CORRECT_WORD_DTYPE)."""
        rows = len(pred_codes)
        assert rows == len(ref_codes) and rows >= 1

        def pack(texts):
            arrs = [np.asarray(t, np.uint8).reshape(-1) for t in texts]
            off = np.zeros(rows + 1, np.int32)
            off[1:] = np.cumsum([len(a) for a in arrs])
            return np.ascontiguousarray(np.concatenate(arrs + [np.zeros(1, np.uint8)])), off

        (pc, po), (rc_, ro) = pack(pred_codes), pack(ref_codes)
        info, ops, words = self._correct_buffers(rows)
        rc = self.lib.qv_correct(self.h, _p(pc), _p(po), _p(rc_), _p(ro), rows, CORRECT_PREFIX if prefix else 0, _p(info), _p(ops),
                                 ops.shape[1], _p(words), words.shape[1], self._stream())
        self._check(rc, "qv_correct")
        return info, ops, words

    def correct(self, pred_texts, ref_texts, prefix: bool = False) -> list[dict]:
        """Word-level comparison of what was heard with what should have been said, on the device (qv_correct): a
        Levenshtein alignment of the two texts' symbols (spaces only separate words) under the reference's tie rule,
        folded into the words of the reference text.  pred_texts / ref_texts: normalised strings (encoded with
        tables.encode) or arrays of alphabet codes, at most 2,048 characters each, at most max_batch rows.  Per row a
        dict of the qv_correct_info fields ("n_ref", "n_pred", "n_words", "n_ref_used", "words_touched", "distance",
        "n_match", "n_sub", "n_del", "n_ins", "n_ops", "flags", "start_verse", "span") plus "ops" (uint8 per alignment
        column: 0 match, 1 substitution, 2 deletion, 3 insertion) and "words" (CORRECT_WORD_DTYPE per reference word).
        prefix=True: the recitation may stop anywhere in the reference (QV_CORRECT_PREFIX).  correction.fold turns a row
        into the reference's list of wrong words."""
        enc = lambda t: self.tables.encode(t) if isinstance(t, str) else np.asarray(t, np.uint8)  # noqa: E731
        return self._corrections(*self.correct_raw([enc(t) for t in pred_texts], [enc(t) for t in ref_texts], prefix))

    def correct_results(self, ctx: int | None = None, batch: int = 1, prefix: bool = False, texts: bool = False) -> list[dict]:
        """The same comparison for every row of context `ctx`'s last batch (default: the most recent call's), entirely from
        what the batch left on the device (qv_correct_results_ctx): the decode stage's normalised transcript against the
        text the winner's tokens were tokenised from, so word k is word k of the word timings.  Rows as correct() returns
        them, "start_verse" / "span" naming the winner; a row without a prediction carries CORRECT_NO_TARGET.
        texts=True adds "pred_codes" (transcript_codes) and "ref_codes" (tables.span_codes), what correction.fold spells
        the wrong words from.  Call it before the context is reused."""
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        info, ops, words = self._correct_buffers(batch)
        rc = self.lib.qv_correct_results_ctx(self.h, int(ctx), int(batch), CORRECT_PREFIX if prefix else 0, _p(info), _p(ops),
                                             ops.shape[1], _p(words), words.shape[1])
        self._check(rc, "qv_correct_results_ctx")
        out = self._corrections(info, ops, words)
        if texts:
            for d, t in zip(out, self.transcript_codes(ctx, batch)):
                d["pred_codes"] = t["codes"]
                d["ref_codes"] = (self.tables.span_codes(d["start_verse"], d["span"]) if d["span"] else np.zeros(0, np.uint8))
        return out

    # ---------------------------------------------------------------- ranked alternatives
    def _with_nbest(self, results: list[dict], nbest: int | None) -> list[dict]:
        if nbest is not None:
            for d, lst in zip(results, self.nbest_results(batch=len(results), k=int(nbest))):
                d["nbest"] = lst
        return results

    def nbest_raw(self, ctx: int | None = None, batch: int = 1, k: int = 5, runners: bool = False):
        """qv_nbest_results_ctx as structured arrays: (info [batch] of NBEST_INFO_DTYPE, entries [batch, k] of
        NBEST_ENTRY_DTYPE)."""
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        info = np.zeros(batch, dtype=NBEST_INFO_DTYPE)
        ent = np.zeros((batch, max(int(k), 1)), dtype=NBEST_ENTRY_DTYPE)
        rc = self.lib.qv_nbest_results_ctx(self.h, int(ctx), int(batch), int(k), NBEST_TEXT_RUNNERS if runners else 0,
                                           _p(info), _p(ent))
        self._check(rc, "qv_nbest_results_ctx")
        return info, ent

    def nbest_results(self, ctx: int | None = None, batch: int = 1, k: int = 5, runners: bool = False) -> list[list[dict]]:
        """Ranked alternatives of every row of context `ctx`'s last batch (default: the most recent call's), selected on
        the device (qv_nbest_results_ctx).  Per row a list of at most k dicts, best first: "surah", "ayah", "ayah_end",
        "start" / "span" (first verse as a global index, number of ayat), "cand_index" (position in the reranked
        candidate list, -1 for text entries), "source", "n_tokens", "score" (the rerank's final_score for a CTC row, the
        text score for a text row), "text_score", "ctc_loss", "ctc_norm_loss".  A reranked row lists the head of the
        rerank's ranking (entry 0 is the prediction); a row decided by the text match lists that match -- with
        runners=True followed by match_verse's runners-up; a row without a prediction is [].  Call it before the context
        is reused."""
        info, ent = self.nbest_raw(ctx, batch, k, runners)
        out = []
        for b in range(batch):
            rows = []
            for e in ent[b, : int(info[b]["n_entries"])]:
                rows.append({"surah": int(e["surah"]), "ayah": int(e["ayah"]), "ayah_end": int(e["ayah_end"]),
                             "start": int(e["start_verse"]), "span": int(e["span"]), "cand_index": int(e["cand_index"]),
                             "source": QV_SOURCE[int(e["source"])], "n_tokens": int(e["n_tokens"]), "score": float(e["score"]),
                             "text_score": float(e["text_score"]), "ctc_loss": float(e["ctc_loss"]),
                             "ctc_norm_loss": float(e["ctc_norm_loss"])})
            out.append(rows)
        return out

    def nbest_select(self, finals, losses, k: int = 5) -> list[list[int]]:
        """The device's selection on explicit vectors (qv_nbest_select): finals[r] (float64) and losses[r] (float32) are
        row r's scores and losses, rows may differ in length (at most 2,048 entries, at most max_batch rows).  Per row
        the indices of the stable top k by score among the entries with a finite loss: score descending, ties to the
        smaller index."""
        rows = len(finals)
        assert rows == len(losses) and rows >= 1
        n = np.ascontiguousarray(np.array([len(x) for x in finals], np.int32))
        assert all(len(a) == len(b) for a, b in zip(finals, losses))
        pitch = max(int(n.max()), 1)
        fin = np.zeros((rows, pitch), np.float64)
        los = np.full((rows, pitch), np.inf, np.float32)
        for r in range(rows):
            fin[r, : n[r]] = np.asarray(finals[r], np.float64)
            los[r, : n[r]] = np.asarray(losses[r], np.float32)
        idx = np.zeros((rows, max(int(k), 1)), np.int32)
        cnt = np.zeros(rows, np.int32)
        rc = self.lib.qv_nbest_select(self.h, _p(fin), _p(los), _p(n), rows, pitch, int(k), _p(idx), _p(cnt), self._stream())
        self._check(rc, "qv_nbest_select")
        assert all((idx[r, cnt[r]:] == -1).all() for r in range(rows))
        return [idx[r, : cnt[r]].tolist() for r in range(rows)]

    # ---------------------------------------------------------------- word timings
    def _with_alignment(self, results: list[dict], align: bool) -> list[dict]:
        if align:
            for d, a in zip(results, self.align_results(batch=len(results))):
                d["alignment"] = a
        return results

    @staticmethod
    def _alignments(info, ids, first, last, logp) -> list[dict]:
        out = []
        for b in range(len(info)):
            flags = int(info[b]["flags"])
            n = 0 if flags else int(info[b]["n_tokens"])
            out.append({"ids": ids[b, :n].astype(np.int32), "first": first[b, :n].astype(np.int32),
                        "last": last[b, :n].astype(np.int32), "logp": logp[b, :n].copy(), "score": float(info[b]["score"]),
                        "flags": flags, "n_tokens": int(info[b]["n_tokens"]), "t_frames": int(info[b]["t_frames"]),
                        "start": int(info[b]["start_verse"]), "span": int(info[b]["span"])})
        return out

    def align(self, log_probs, t_frames, targets) -> list[dict]:
        """CTC forced alignment (qv_align) of explicit token lists: targets[b] (ids 0..1023) against row b of the float32
        cuda tensor log_probs [B, t_max, 1025] with t_frames[b] valid frames.  Per row a dict: "ids", "first", "last"
        (first / last encoder frame of every token, inclusive; a frame is 0.08 s), "logp" (mean log-prob of the token over
        its frames), "score" (log-prob of the whole path), "flags" (ALIGN_NO_TARGET / ALIGN_TOO_LONG / ALIGN_INFEASIBLE:
        the arrays are then empty and score is 0), "n_tokens", "t_frames"."""
        B, t_max, t = self._logprob_args(log_probs, t_frames)
        assert len(targets) == B
        lens = np.ascontiguousarray(np.array([len(x) for x in targets], np.int32))
        tg = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint16).reshape(-1) for x in targets] + [np.zeros(1, np.uint16)]))
        pitch = ALIGN_MAX_TOKENS
        info = np.zeros(B, dtype=ALIGN_INFO_DTYPE)
        first, last = np.zeros((B, pitch), np.int16), np.zeros((B, pitch), np.int16)
        logp = np.zeros((B, pitch), np.float32)
        rc = self.lib.qv_align(self.h, C.c_void_p(log_probs.data_ptr()), _p(t), B, t_max, _p(tg), _p(lens), _p(info), _p(first), _p(last),
                               _p(logp), pitch, self._stream())
        self._check(rc, "qv_align")
        ids = np.full((B, pitch), -1, np.int32)
        for b, x in enumerate(targets):
            if not info[b]["flags"]:
                ids[b, : len(x)] = np.asarray(x, np.int32)
        return self._alignments(info, ids, first, last, logp)

    def align_results(self, ctx: int | None = None, batch: int = 1) -> list[dict]:
        """Forced alignment of the winners of context `ctx`'s last batch (default: the most recent call's) against the
        log-probs that batch was decoded from (qv_align_results_ctx): dicts as align() returns, plus "start" / "span" --
        the winner's first verse (global index) and number of ayat; "ids" are the table's token ids of that text
        (tables.token_ids(start, span)).  Rows without a prediction carry ALIGN_NO_TARGET.  Call it before the context is
        reused; after decode_retrieve_rerank the caller's log-prob tensor must still be alive."""
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        pitch = ALIGN_MAX_TOKENS
        info = np.zeros(batch, dtype=ALIGN_INFO_DTYPE)
        ids = np.zeros((batch, pitch), np.uint16)
        first, last = np.zeros((batch, pitch), np.int16), np.zeros((batch, pitch), np.int16)
        logp = np.zeros((batch, pitch), np.float32)
        rc = self.lib.qv_align_results_ctx(self.h, int(ctx), int(batch), _p(info), _p(ids), _p(first), _p(last), _p(logp), pitch)
        self._check(rc, "qv_align_results_ctx")
        return self._alignments(info, ids, first, last, logp)

    def predict_batch_async(self, audio, lengths):
        B, N, ln = self._audio_args(audio, lengths)
        ctx = C.c_int32(-1)
        rc = self.lib.qv_predict_batch_async_ctx(self.h, C.c_void_p(audio.data_ptr()), _p(ln), B, N, self._stream(), C.byref(ctx))
        self._check(rc, "qv_predict_batch_async_ctx")
        return int(ctx.value)     # (the id comes back from the call itself: another thread cannot get in between)

    def fetch_results(self, ctx: int, batch: int, t_max: int, want_text: bool = False) -> list[dict]:
        """join context `ctx` (the value predict_batch_async returned) and copy its results out."""
        res = np.zeros(batch, dtype=RESULT_DTYPE)
        greedy = np.full((batch, t_max), -1, dtype=np.int32) if want_text else None
        rc = self.lib.qv_fetch_results_ctx(self.h, ctx, batch, t_max, _p(res), _p(greedy))
        self._check(rc, "qv_fetch_results_ctx")
        return self._results(res, greedy)

    def wait(self, ctx: int):
        """host-side join of context `ctx` (the value predict_batch_async returned): returns when its batch is done."""
        self._check(self.lib.qv_wait_ctx(self.h, int(ctx)), "qv_wait_ctx")

    def packed_results(self, batch: int, ctx: int | None = None):
        """int32 cuda tensor [batch, 4] = (surah, ayah, ayah_end, float-bits(score)) of the last
        async call -- or, with batches in flight, of context `ctx` (joined on the current stream).
        This is the payload of the per-batch all-gather."""
        torch = self.torch
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        ptr = self.lib.qv_packed_results_ctx(self.h, ctx, self._stream())
        if not ptr:
            raise QvError("qv_packed_results_ctx failed")
        out = torch.empty((batch, 4), dtype=torch.int32, device=f"cuda:{self.device}")
        # device-to-device copy out of the engine-owned buffer on the current stream
        import ctypes

        hip = _hip_runtime()
        rc = hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(ptr), batch * 16, 3, self._stream())
        if rc != 0:
            raise QvError(f"hipMemcpyAsync failed ({rc})")
        return out

    def resample_poly(self, x, up: int, down: int):
        """scipy.signal.resample_poly(x, up, down) for a float32 cuda vector, computed on the GPU
        and bit-identical to scipy's float32 result (a15: the TTA wrapper's 0.9x / 1.1x speed
        perturbation, c2c-direct-mixed-tta/run.py:60-71)."""
        from .audio import resample_plan

        torch = self.torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()
        n_in = int(x.numel())
        up, down, taps, m0, n_out = resample_plan(up, down, n_in)
        if up == down == 1:
            return x.clone()
        y = torch.empty(n_out, dtype=torch.float32, device=x.device)
        rc = self.lib.qv_upfirdn(self.h, C.c_void_p(x.data_ptr()), n_in, _p(taps), len(taps),
                                 up, down, m0, n_out, C.c_void_p(y.data_ptr()), self._stream())
        self._check(rc, "qv_upfirdn")
        return y

    RESAMPLE_ROWS = 1024   # rows per qv_upfirdn_batch / qv_mixdown_batch call (QV_RESAMPLE_ROWS)

    def resample_rows(self, x, lengths, up: int, down: int, src_rows=None, out_pitch: int | None = None):
        """scipy.signal.resample_poly(row, up, down) for every row of a float32 cuda matrix in ONE launch (qv_upfirdn_batch;
        one launch per 1,024 rows, all into the same output): x [R0, pitch] holds the clips zero-padded, ``lengths`` their
        sample counts; ``src_rows`` (optional) picks which rows of x are resampled (output row r <- x[src_rows[r]],
        lengths[r] = that clip's length).  Returns (y [R, out_pitch] zero-padded like x, list of output lengths).  Every
        output sample is bit-identical to resample_poly's float32 one."""
        from .audio import resample_plan

        torch = self.torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
        rows = len(lens)
        plan = [resample_plan(up, down, int(n)) for n in sorted(set(lens.tolist()))]
        up_r, down_r, m0 = plan[0][0], plan[0][1], plan[0][3]
        if up_r == down_r == 1:
            y = x if src_rows is None else x[torch.as_tensor(list(src_rows), device=x.device)]
            return y.clone(), lens.tolist()
        # one filter for the whole batch: the longest zero padding any row's length asks for (padding taps add exact zeros)
        taps = max((p[2] for p in plan), key=len)
        n_out = [int((int(n) * up_r + down_r - 1) // down_r) for n in lens]
        pitch = int(out_pitch or max(n_out))
        assert pitch >= max(n_out)
        y = torch.empty((rows, pitch), dtype=torch.float32, device=x.device)
        src = None if src_rows is None else np.ascontiguousarray(np.asarray(list(src_rows), dtype=np.int32))
        x_pitch = int(x.stride(0))
        for r0 in range(0, rows, self.RESAMPLE_ROWS):     # the C ABI takes 1,024 rows a call: chunks of one output tensor
            r1 = min(rows, r0 + self.RESAMPLE_ROWS)
            ln_c = lens[r0:r1]
            src_c = None if src is None else src[r0:r1]
            x_ptr = x.data_ptr() + (0 if src is not None else r0 * x_pitch * 4)   # without src_rows a chunk's row 0 is row r0 of x
            rc = self.lib.qv_upfirdn_batch(self.h, C.c_void_p(x_ptr), x_pitch, _p(src_c), _p(ln_c), r1 - r0, _p(taps), len(taps),
                                           up_r, down_r, m0, C.c_void_p(y.data_ptr() + r0 * pitch * 4), pitch, self._stream())
            self._check(rc, "qv_upfirdn_batch")
        return y, n_out

    def mixdown_rows(self, x, n_frames, channels: int):
        """interleaved [R, frames * channels] float32 cuda rows -> mono [R, max frames]: numpy's float32 mean over the channels,
        the frame's sum taken in numpy's own order (left to right below 8 channels, eight running sums joined by a fixed tree
        plus the tail from 8 up: k_mixdown), an all -0.0 frame giving +0.0 as numpy's does.  One launch per 1,024 rows."""
        torch = self.torch
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        nf = np.ascontiguousarray(np.asarray(n_frames, dtype=np.int64))
        y = torch.zeros((len(nf), int(nf.max())), dtype=torch.float32, device=x.device)
        x_pitch, y_pitch = int(x.stride(0)), int(y.stride(0))
        for r0 in range(0, len(nf), self.RESAMPLE_ROWS):
            nf_c = nf[r0:r0 + self.RESAMPLE_ROWS]
            rc = self.lib.qv_mixdown_batch(self.h, C.c_void_p(x.data_ptr() + r0 * x_pitch * 4), x_pitch, _p(nf_c), len(nf_c), int(channels),
                                           C.c_void_p(y.data_ptr() + r0 * y_pitch * 4), y_pitch, self._stream())
            self._check(rc, "qv_mixdown_batch")
        return y

    def speed_perturb_rows(self, x, lengths, factor: float, src_rows=None):
        """the TTA wrapper's speed perturbation (tta/run.py:60-71: up = int(factor * 10), down = 10) of many clips at once"""
        return self.resample_rows(x, lengths, int(factor * 10), 10, src_rows=src_rows)

    def speed_perturb(self, x, factor: float):
        """0.9 = 10 % slower, 1.1 = 10 % faster (tta/run.py:60-71: up = int(factor * 10), down = 10)."""
        return x if factor == 1.0 else self.resample_poly(x, int(factor * 10), 10)

    # ---------------------------------------------------------------- measurement
    GEMM_EPILOGUES = ["f16", "f16_swish", "f16_relu", "glu", "resid", "f32", "qkv"]

    def gemm_tiles(self, mode: int):
        """process-wide GEMM tile policy (qv_debug_gemm_tiles): 0 = 128-wide only, 1 = default, 2 = 256 x 256
        wherever the shape allows, -1 = environment / default."""
        self._check(self.lib.qv_debug_gemm_tiles(int(mode)), "qv_debug_gemm_tiles")

    def gemm_tile_height(self, mode: int):
        """tile height of the wide GEMM kernel (qv_debug_gemm_tile_height): 0 = 256 rows always, 1 = default (192 rows where
        they save a round of tiles and < 3 batches are in flight), 2 = that rule always, 3 = 192 rows always, -1 = env / default."""
        self._check(self.lib.qv_debug_gemm_tile_height(int(mode)), "qv_debug_gemm_tile_height")

    def gemm_pipeline(self, ld: int = -1, nst: int = -1, narrow: int = -1):
        """process-wide pipeline of the 128- / 64-wide GEMM kernels (qv_debug_gemm_pipeline; QVERSE_GEMM_LD / _NST / _NARROW):
        ld 1 = register-staged loaders (default), 0 = direct global->LDS loads; nst = LDS stages of the direct loads (2..4,
        0 = from the shape); narrow 1 / 0 = 64- / 128-wide tiles where the kernel exists; -1 = environment / default."""
        self._check(self.lib.qv_debug_gemm_pipeline(int(ld), int(nst), int(narrow)), "qv_debug_gemm_pipeline")

    def replay_kernel(self, which: int) -> str:
        """name of the kernel the launcher picks for layer-0 GEMM `which` (REPLAY_SHAPES) at the last forward's row count
        under the current switches (qv_profile_replay_kernel); launches nothing."""
        name = C.create_string_buffer(64)
        self._check(self.lib.qv_profile_replay_kernel(self.h, which, name, 64), "qv_profile_replay_kernel")
        return name.value.decode()

    def weights_info(self) -> str:
        """precision mode and where the quantisation grids came from (qv_weights_info)"""
        buf = C.create_string_buffer(512)
        self._check(self.lib.qv_weights_info(self.h, buf, 512), "qv_weights_info")
        return buf.value.decode()

    def attention_variant(self, mode: int):
        """process-wide attention kernel variant (qv_debug_attention_variant): 3 = default (utterances of <= 128 frames on
        the single-pass kernel, longer ones on the loader-wave key-tiled kernel), 0 = that kernel with two heads per block for
        every utterance, 1 = one head per block, 2 = one wave per query tile, 4 = k_attention_x for every utterance,
        5 = single-pass + k_attention_x (0, 1, 2, 4: identical bits; 3, 5: identical bits), -1 = environment / default."""
        self._check(self.lib.qv_debug_attention_variant(int(mode)), "qv_debug_attention_variant")

    def kernel_variant(self, which: int, mode: int):
        """process-wide variant of one kernel (qv_debug_kernel_variant): which 0 = log-mel FFT (0 LDS, 1 registers, 2 registers and a wave walks a run of frames),
        1 = precision 2's conv.0 (0 VALU, 1 f32 matrix pipe), 2 = span pass (0 one walk per span, 1 prefix-shared),
        3 = forward of a multi-context engine (0 plain launches, 1 hipGraph replay of a repeating shape),
        5 = tiles of four conv.2 frames a block of the fused subsampling kernel walks (0 from the launch shape, 1 / 2 tiles,
        3 the maximum, 4 the maximum with the run's mel rows resident in LDS), 6 = steps of three conv.5 frames a block of the conv.3 + conv.5 kernel walks (same codes);
        -1 = environment / default.  Identical bits either way."""
        self._check(self.lib.qv_debug_kernel_variant(int(which), int(mode)), "qv_debug_kernel_variant")

    def forward_graph_stats(self) -> dict:
        """forwards replayed as one hipGraph launch / graphs captured since the engine was created."""
        r, c = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.qv_debug_forward_graph_stats(self.h, C.byref(r), C.byref(c)), "qv_debug_forward_graph_stats")
        return {"replays": int(r.value), "captures": int(c.value)}

    def profile_gemm(self, enable: bool):
        self._check(self.lib.qv_profile_gemm(self.h, int(enable)), "qv_profile_gemm")

    def profile_gemm_read(self) -> list[dict]:
        """per GEMM kernel class: summed HIP-event ms, algorithmic FLOPs, launches."""
        ms = np.zeros(21)
        fl = np.zeros(21)
        n = np.zeros(21, np.int32)
        self._check(self.lib.qv_profile_gemm_read(self.h, _p(ms), _p(fl), _p(n)), "qv_profile_gemm_read")
        out = []
        for c in range(21):
            if n[c]:
                epi, tile = self.GEMM_EPILOGUES[c // 3], c % 3
                out.append({"kernel": f"k_gemm256<{epi}>" if tile == 2 else f"k_gemm<{epi},{128 if tile else 64}>",
                            "ms": float(ms[c]), "flops": float(fl[c]), "launches": int(n[c])})
        return out

    def inject_logprobs(self, log_probs=None, t_frames=None):
        """measurement hook (qv_profile_inject_logprobs): the post-logits stages of predict_batch_async read this cuda
        tensor [B, t_max, 1025] instead of the forward's output (the forward still runs); None clears it.  The tensor is
        kept alive by the engine object."""
        if log_probs is None:
            self._injected = None
            self._check(self.lib.qv_profile_inject_logprobs(self.h, None, 0, None, 0), "qv_profile_inject_logprobs")
            return
        B, t_max, t = self._logprob_args(log_probs, t_frames, per_row=False)
        self._injected = log_probs
        self._check(self.lib.qv_profile_inject_logprobs(self.h, C.c_void_p(log_probs.data_ptr()), t_max, _p(t), B), "qv_profile_inject_logprobs")

    def profile_stages(self, enable: bool):
        """device-side stage timers (the reference's C2C_DIRECT_MIXED_PROFILE split, mixed/run.py:117-124)"""
        self._check(self.lib.qv_profile_stages(self.h, int(enable)), "qv_profile_stages")

    def stage_times(self, ctx: int | None = None) -> dict:
        """seconds spent in forward / decode / build / rerank by the last batch of context `ctx`
        (default: the most recent call's); waits for that batch."""
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        ms = np.zeros(4, np.float32)
        self._check(self.lib.qv_stage_times(self.h, ctx, _p(ms)), "qv_stage_times")
        return {k: float(v) * 1e-3 for k, v in zip(("forward", "decode", "build", "rerank"), ms)}

    REPLAY_SHAPES = ["FFN-up [M,512]x[512,2048]+Swish", "FFN-down [M,2048]x[2048,512]+residual", "QKV [M,512]x[512,1536]",
                     "attention out [M,512]x[512,512]+residual", "pointwise conv [M,512]x[512,1024]+GLU"]

    def replay_gemm(self, which: int, iters: int = 50) -> dict:
        """average duration (HIP events on the launch stream) of `iters` back-to-back launches of one
        layer-0 GEMM with the shapes of the last forward."""
        us, fl = C.c_double(), C.c_double()
        self._check(self.lib.qv_profile_replay_gemm(self.h, which, iters, C.byref(us), C.byref(fl), self._stream()),
                    "qv_profile_replay_gemm")
        name = C.create_string_buffer(64)
        self._check(self.lib.qv_profile_replay_kernel(self.h, which, name, 64), "qv_profile_replay_kernel")
        return {"kernel": name.value.decode(), "shape": self.REPLAY_SHAPES[which], "avg_us": us.value,
                "flops": fl.value, "launches": iters}

    # ---------------------------------------------------------------- debug ------
    # ---------------------------------------------------------------- streaming row
    def next_verse(self, surah: int, ayah: int) -> int:
        """Global index of the verse after (surah, ayah) in mushaf order, -1 if there is none
        or (surah, ayah) does not exist (QuranDB.get_next_verse, shared/quran_db.py:81-90)."""
        t = self.tables.s
        if not (1 <= surah <= 114) or not (1 <= ayah <= int(t["surah_len"][surah - 1])):
            return -1
        idx = int(t["surah_start"][surah - 1]) + ayah - 1
        return idx + 1 if idx + 1 < self.tables.n_verses else -1

    def track_match(self, texts, last_refs=None) -> list[dict | None]:
        """VerseTracker._find_best_match for a batch of accumulated texts in one launch
        (qv_tracker_match).  last_refs[b] = (surah, ayah) of the tracker's last emission or None.
        Returns per text None (no verse scores above 0) or
        {surah, ayah, n_words, score, verse, variant}; the caller applies its emit gates."""
        n = len(texts)
        if n == 0:
            return []
        last_refs = last_refs or [None] * n
        texts = [front_window(t, self.max_transcript) for t in texts]   # beyond the engine's window: matched on the front window
        enc = [self.tables.encode(t) for t in texts]
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(e) for e in enc])
        codes = np.ascontiguousarray(np.concatenate(enc) if off[-1] else np.zeros(1, np.uint8))
        nw = np.ascontiguousarray(np.array([len(t.split()) for t in texts], np.int32))
        bonus = np.ascontiguousarray(np.array([self.next_verse(*r) if r else -1 for r in last_refs], np.int32))
        out = (QvTrackMatch * n)()
        rc = self.lib.qv_tracker_match(self.h, _p(codes), _p(off), _p(nw), _p(bonus), n, C.cast(out, C.c_void_p),
                                       self._stream())
        self._check(rc, "qv_tracker_match")
        return [None if m.verse < 0 else
                {"surah": m.surah, "ayah": m.ayah, "n_words": m.n_words, "score": m.score, "verse": m.verse,
                 "variant": m.variant} for m in out]

    def continuation_bonuses(self, hint) -> list[tuple[int, float]]:
        """QuranDB._continuation_bonuses (shared/quran_db.py:121-146) as (verse index, bonus)
        pairs: the three ayat after the hint, or - when the hint is the last ayah of its surah -
        the first three of the next surah."""
        if not hint:
            return []
        s, a = hint
        t = self.tables.s
        n_surah = len(t["surah_len"])

        def idx(su, ay):
            if 1 <= su <= n_surah and 1 <= ay <= int(t["surah_len"][su - 1]):
                return int(t["surah_start"][su - 1]) + ay - 1
            return None

        out = []
        if idx(s, a + 1) is not None:
            for k, bonus in enumerate((0.22, 0.12, 0.06)):
                i = idx(s, a + 1 + k)
                if i is not None:
                    out.append((i, bonus))
        elif 1 <= s + 1 <= n_surah:
            first = int(t["surah_start"][s])
            for k, bonus in zip(range(min(3, int(t["surah_len"][s]))), (0.22, 0.12, 0.06)):
                out.append((first + k, bonus))
        return out

    def match_verse(self, text: str, threshold: float = 0.3, max_span: int = 3, hint=None) -> dict | None:
        """QuranDB.match_verse without the trigram restriction (qv_match_verse).  Returns None
        below the threshold, else {surah, ayah, ayah_end (None for one ayah), score, n_words}
        where n_words counts the words of the matched text_clean (what the caller trims by)."""
        text = normalize_arabic(text)
        if not text.strip():
            return None
        codes = np.ascontiguousarray(self.tables.encode(front_window(text, self.max_transcript)))
        bon = self.continuation_bonuses(hint)
        bv = np.ascontiguousarray(np.array([b[0] for b in bon] + [0] * (3 - len(bon)), np.int32))
        bb = np.ascontiguousarray(np.array([b[1] for b in bon] + [0.0] * (3 - len(bon)), np.float64))
        st, sp, sc = C.c_int32(), C.c_int32(), C.c_double()
        rc = self.lib.qv_match_verse(self.h, _p(codes), len(codes), len(bon), _p(bv), _p(bb), int(max_span),
                                     C.byref(st), C.byref(sp), C.byref(sc), self._stream())
        self._check(rc, "qv_match_verse")
        if st.value < 0 or not (sc.value >= threshold):
            return None
        v, span = st.value, sp.value
        t = self.tables.s
        if span == 1:
            n_words = int(t["clean_nw"][v])
        else:
            first = int(t["nobsm_nw"][v]) or int(t["clean_nw"][v])
            n_words = first + sum(int(t["clean_nw"][v + k]) for k in range(1, span))
        s, a = int(self.tables.surah[v]), int(self.tables.ayah[v])
        return {"surah": s, "ayah": a, "ayah_end": a + span - 1 if span > 1 else None, "score": sc.value,
                "n_words": n_words, "verse": v, "span": span}

    def _transcripts(self, info, ids, logp, first, last) -> list[dict]:
        out = []
        # (whole arrays to Python objects at once: per-element numpy scalar access would cost more than the device call)
        for b, (n, t, n_blank, flags, mn, _, avg, favg) in enumerate(info.tolist()):
            row = ids[b, :n].tolist()
            out.append({
                "text": self.transcript_of(row),
                "avg_logprob": avg, "frame_avg_logprob": favg, "min_token_logprob": mn, "n_tokens": n, "t_frames": t,
                "n_blank_frames": n_blank, "flags": flags,
                "tokens": [{"id": i, "first": f, "last": l, "logp": p}
                           for i, f, l, p in zip(row, first[b, :n].tolist(), last[b, :n].tolist(), logp[b, :n].tolist())],
            })
        return out

    def transcribe_raw(self, log_probs, t_frames, pitch: int | None = None):
        """qv_transcribe as arrays: (info [B] of TRANSCRIPT_INFO_DTYPE, ids int32 [B, pitch], logp float32, first / last
        int16 [B, pitch]); entries past a row's n_tokens hold -1 (ids, first, last) and 0 (logp)."""
        B, t_max, t = self._logprob_args(log_probs, t_frames)
        head = (C.c_void_p(log_probs.data_ptr()), _p(t), B, t_max)
        return self._transcribe_call(self.lib.qv_transcribe, "qv_transcribe", head, B, t_max if pitch is None else int(pitch))

    def _transcribe_call(self, fn, what, head, B, pitch):
        info = np.zeros(B, dtype=TRANSCRIPT_INFO_DTYPE)
        ids = np.zeros((B, max(pitch, 1)), np.int32)
        logp = np.zeros((B, max(pitch, 1)), np.float32)
        first, last = np.zeros((B, max(pitch, 1)), np.int16), np.zeros((B, max(pitch, 1)), np.int16)
        self._check(fn(self.h, *head, _p(info), _p(ids), _p(logp), _p(first), _p(last), pitch, self._stream()), what)
        return info, ids, logp, first, last

    def transcribe_logprobs(self, log_probs, t_frames) -> list[dict]:
        """Greedy transcription with confidence (qv_transcribe) of float32 cuda log-probs [B, t_max, 1025] with t_frames[b]
        valid frames.  Per row a dict: "text" (transcript_of the ids), "avg_logprob" (mean over the tokens of each token's
        best frame), "frame_avg_logprob" (mean over the frames of the frame's maximum), "min_token_logprob", "n_tokens",
        "t_frames", "n_blank_frames", "flags", and "tokens": [{"id", "first", "last" (encoder frames, inclusive; a frame is
        0.08 s), "logp"}].  One kernel, one copy back; definitions in include/qverse.h."""
        return self._transcripts(*self.transcribe_raw(log_probs, t_frames))

    def transcribe_batch(self, audio, lengths, confidence: bool = False):
        """Forward + greedy CTC decode of a zero-padded batch (float32 cuda [B, N]); the
        transcript of each row as c2c-direct/run.py:187-204 returns it.  confidence=True: one dict per row as
        transcribe_logprobs returns it (qv_transcribe_batch: the forward into the engine's own workspace, argmax, collapse
        and confidence on the device) -- a reference-style {"text", "avg_logprob"} transcriber result."""
        if confidence:
            B, N, ln = self._audio_args(audio, lengths)
            head = (C.c_void_p(audio.data_ptr()), _p(ln), B, N)   # (the pitch: the longest row's frames, never below 1)
            return self._transcripts(*self._transcribe_call(self.lib.qv_transcribe_batch, "qv_transcribe_batch", head, B,
                                                            self.frames_for(int(ln.max()))))
        lp, T = self.forward(audio, lengths)
        ids = lp.argmax(-1).cpu().numpy()
        out = []
        for b, t in enumerate(T):
            row = ids[b, :t]
            keep = np.ones(t, bool)
            keep[1:] = row[1:] != row[:-1]
            out.append(self.transcript_of(row[keep & (row != 1024)].tolist()))
        return out

    # ------------------------------------------------ verse-constrained beam search -----
    def trie_node_tokens(self, node: int, max_span: int = 3) -> list[int]:
        """the tokens from the root to `node` of the trie for max_span (qv_trie_node_tokens)"""
        ids = np.zeros(1024, np.int32)
        n = C.c_int32(0)
        rc = self.lib.qv_trie_node_tokens(self.h, int(max_span), int(node), _p(ids), len(ids), C.byref(n))
        self._check(rc, "qv_trie_node_tokens")
        return ids[: n.value].tolist()

    def beam_raw(self, log_probs, t_frames, beam: int = 8, k: int = 5, max_span: int = 3):
        """qv_beam_decode as arrays: (info [B] of BEAM_INFO_DTYPE, entries [B, k] of BEAM_ENTRY_DTYPE, ids int32 [B, t_max] --
        the tokens of entry 0, -1 padded)."""
        B, t_max, t = self._logprob_args(log_probs, t_frames)
        head = (C.c_void_p(log_probs.data_ptr()), _p(t), B, t_max)
        return self._beam_call(self.lib.qv_beam_decode, "qv_beam_decode", head, B, t_max, beam, k, max_span)

    def _beam_call(self, fn, what, head, B, pitch, beam, k, max_span):
        info = np.zeros(B, dtype=BEAM_INFO_DTYPE)
        ent = np.zeros((B, max(int(k), 1)), dtype=BEAM_ENTRY_DTYPE)
        ids = np.full((B, max(pitch, 1)), -1, np.int32)
        self._check(fn(self.h, *head, int(max_span), int(beam), int(k), _p(info), _p(ent), _p(ids), pitch, self._stream()), what)
        return info, ent, ids

    def _beam_rows(self, info, ent, ids, max_span: int) -> list[dict]:
        tab = self.tables
        out = []
        for b in range(len(info)):
            hyps = []
            for i, e in enumerate(ent[b, : int(info[b]["n_entries"])].tolist()):
                (node, n_tok, n_ends, start, span, surah, ayah, ayah_end, below, bv, bs, flags, score, pb, pnb) = e
                toks = ids[b, :n_tok].tolist() if i == 0 else self.trie_node_tokens(node, max_span)
                first = (int(tab.surah[bv]), int(tab.ayah[bv]), int(tab.ayah[bv]) + bs - 1) if below else None
                hyps.append({"surah": surah, "ayah": ayah, "ayah_end": ayah_end if surah else None, "score": score,
                             "complete": bool(flags & BEAM_COMPLETE), "n_tokens": n_tok, "text": tab.ids_to_text(toks),
                             "matches": n_ends, "reachable": below, "first_reachable": first, "node": node, "start": start,
                             "span": span, "blank_score": pb, "nonblank_score": pnb, "ids": toks})
            out.append({"t_frames": int(info[b]["t_frames"]), "max_candidates": int(info[b]["max_candidates"]), "hypotheses": hyps})
        return out

    def beam_logprobs(self, log_probs, t_frames, beam: int = 8, k: int = 5, max_span: int = 3) -> list[dict]:
        """Verse-constrained CTC prefix beam search (qv_beam_decode; definition in include/qverse.h) of float32 cuda log-probs
        [B, t_max, 1025] with t_frames[b] valid frames: every hypothesis is a prefix of a verse or of up to max_span
        consecutive verses.  Per row {"t_frames", "max_candidates", "hypotheses"}; the at most k hypotheses, best first, are
        {"surah", "ayah", "ayah_end" (of the first verse run that ENDS at the prefix; 0, 0, None when none does), "score"
        (log-probability of the prefix), "complete", "n_tokens", "text" (Tables.ids_to_text of the prefix), "matches" (verse
        runs that end here), "reachable" (verse runs that start with the prefix), "first_reachable" (surah, ayah, ayah_end of
        the first of them), and "node", "start", "span", "blank_score", "nonblank_score", "ids"}."""
        return self._beam_rows(*self.beam_raw(log_probs, t_frames, beam, k, max_span), max_span)

    def beam_batch(self, audio, lengths, beam: int = 8, k: int = 5, max_span: int = 3) -> list[dict]:
        """beam_logprobs behind the forward (qv_beam_batch): audio float32 cuda [B, N], zero padded"""
        B, N, ln = self._audio_args(audio, lengths)
        head = (C.c_void_p(audio.data_ptr()), _p(ln), B, N)
        pitch = max(self.frames_for(int(ln.max())), 1)
        return self._beam_rows(*self._beam_call(self.lib.qv_beam_batch, "qv_beam_batch", head, B, pitch, beam, k, max_span), max_span)

    # ------------------------------------------------ exhaustive CTC scan -----
    def _scan_masks(self, surahs, B: int) -> np.ndarray | None:
        """surahs: None (every surah), an iterable of surah numbers for all rows, or one such iterable (or None) per row
        -> uint32 [B, 4] or None"""
        if surahs is None:
            return None
        surahs = list(surahs)
        per_row = len(surahs) == B and all(s is None or not isinstance(s, (int, np.integer)) for s in surahs)
        rows = surahs if per_row else [surahs] * B
        out = np.empty((B, 4), np.uint32)
        for b, s in enumerate(rows):
            m = surah_mask(s)
            out[b] = 0xFFFFFFFF if m is None else m
        return np.ascontiguousarray(out)

    def _scan_rows(self, info, ent, losses) -> list[dict]:
        out = []
        for b in range(len(info)):
            cands = [dict(zip(SCAN_ENTRY_DTYPE.names, e)) for e in ent[b, : int(info[b]["n_entries"])].tolist()]
            row = {"t_frames": int(info[b]["t_frames"]), "n_feasible": int(info[b]["n_feasible"]),
                   "n_recursions": int(info[b]["n_recursions"]), "candidates": cands}
            if losses is not None:
                row["losses"] = losses[b]
            out.append(row)
        return out

    def scan_raw(self, log_probs, t_frames, k: int = 5, max_span: int = 6, span_penalty: float | None = None, surahs=None,
                 return_losses: bool = False):
        """qv_scan_logprobs as arrays: (info [B] of SCAN_INFO_DTYPE, entries [B, k] of SCAN_ENTRY_DTYPE, losses -- a float32
        cuda tensor [B, n_verses * 6] with +inf at every key that was not scored, or None)."""
        B, t_max, t = self._logprob_args(log_probs, t_frames)
        head = (C.c_void_p(log_probs.data_ptr()), _p(t), B, t_max)
        return self._scan_call(self.lib.qv_scan_logprobs, "qv_scan_logprobs", head, B, log_probs.device, k, max_span, span_penalty, surahs,
                               return_losses)

    def _scan_call(self, fn, what, head, B, device, k, max_span, span_penalty, surahs, return_losses):
        torch = self.torch
        info = np.zeros(B, dtype=SCAN_INFO_DTYPE)
        ent = np.zeros((B, max(int(k), 1)), dtype=SCAN_ENTRY_DTYPE)
        mask = self._scan_masks(surahs, B)
        losses = torch.empty((B, self.tables.n_verses * 6), dtype=torch.float32, device=device) if return_losses else None
        pen = float(self.cfg.span_penalty if span_penalty is None else span_penalty)
        rc = fn(self.h, *head, int(max_span), pen, int(k), _p(mask), _p(info), _p(ent),
                C.c_void_p(losses.data_ptr()) if return_losses else None, self._stream())
        self._check(rc, what)
        return info, ent, losses

    def scan_logprobs(self, log_probs, t_frames, k: int = 5, max_span: int = 6, span_penalty: float | None = None, surahs=None,
                      return_losses: bool = False) -> list[dict]:
        """Exhaustive CTC scan (qv_scan_logprobs; definition in include/qverse.h) of float32 cuda log-probs [B, t_max, 1025]
        with t_frames[b] valid frames: every verse and every run of up to max_span ayat whose 2 L + 1 states fit the frames
        is CTC-scored, the best k by -loss / L - span_penalty * (span - 1) come back.  span_penalty None = the engine's
        CTC_DIRECT_SPAN_PENALTY; surahs: None, surah numbers for all rows, or one list (or None) per row.  Per row
        {"t_frames", "n_feasible", "n_recursions", "candidates": [{"start_verse", "span", "surah", "ayah", "ayah_end",
        "n_tokens", "loss", "norm", "final_score"}]}, and with return_losses "losses": the row of the float32 cuda tensor
        [B, n_verses * 6] that holds every scored key's loss at verse * 6 + span - 1 and +inf elsewhere."""
        return self._scan_rows(*self.scan_raw(log_probs, t_frames, k, max_span, span_penalty, surahs, return_losses))

    def scan_batch(self, audio, lengths, k: int = 5, max_span: int = 6, span_penalty: float | None = None, surahs=None,
                   return_losses: bool = False) -> list[dict]:
        """scan_logprobs behind the forward (qv_scan_batch): audio float32 cuda [B, N], zero padded"""
        B, N, ln = self._audio_args(audio, lengths)
        head = (C.c_void_p(audio.data_ptr()), _p(ln), B, N)
        return self._scan_rows(*self._scan_call(self.lib.qv_scan_batch, "qv_scan_batch", head, B, audio.device, k, max_span, span_penalty,
                                                surahs, return_losses))

    def scan_kernel_times(self) -> dict:
        """with profile_stages(True): seconds the last scan spent in its two kernels (qv_scan_kernel_times)"""
        ms = np.zeros(2, np.float32)
        self._check(self.lib.qv_scan_kernel_times(self.h, _p(ms)), "qv_scan_kernel_times")
        return {"score": float(ms[0]) * 1e-3, "select": float(ms[1]) * 1e-3}

    # ------------------------------------------------ recordings of any length -----
    def _long_args(self, window_s, margin_s) -> tuple[int, int]:
        """(window_samples, margin_frames) as the C calls take them: seconds to whole frames of 1280 samples; None = the
        environment's value (QVERSE_LONG_WINDOW_S / QVERSE_LONG_MARGIN_S), else the library's default (0 / -1)"""
        env_w, env_m = long_env()
        window_s = env_w if window_s is None else window_s
        margin_s = env_m if margin_s is None else margin_s
        window = 0 if window_s is None else int(round(float(window_s) * 16000)) // QV_LONG_HOP * QV_LONG_HOP
        margin = -1 if margin_s is None else int(round(float(margin_s) * 16000 / QV_LONG_HOP))
        if window_s is not None and window < QV_LONG_HOP:
            raise QvError(f"long window of {window_s} s is shorter than one frame of {QV_LONG_HOP} samples")
        return window, margin

    def long_plan_raw(self, n_samples: int, window_samples: int = 0, margin_frames: int = -1) -> dict:
        """qv_long_plan for this engine's max_samples (include/qverse.h, "recordings of any length"); host only"""
        out = [C.c_int32() for _ in range(4)]
        rc = self.lib.qv_long_plan(int(n_samples), self.max_samples, int(window_samples), int(margin_frames), *map(C.byref, out))
        if rc != 0:
            raise QvError(f"qv_long_plan failed ({rc}): n = {n_samples}, window_samples = {window_samples}, margin_frames = {margin_frames}")
        nw, t, kw, m = (int(v.value) for v in out)
        return {"n_windows": nw, "t_frames": t, "kw": kw, "margin_frames": m, "hop_frames": kw - 2 * m, "window_samples": kw * QV_LONG_HOP}

    def long_plan(self, n: int, window_s: float | None = None, margin_s: float | None = None) -> dict:
        """How a recording of n samples is cut: {"n_windows", "t_frames", "kw", "margin_frames", "hop_frames", "window_samples"}"""
        return self.long_plan_raw(n, *self._long_args(window_s, margin_s))

    def _long_call(self, fn, what, head, rows, t_top, window_samples, margin_frames, pitch):
        pitch = t_top if pitch is None else int(pitch)
        info = np.zeros(rows, dtype=LONG_INFO_DTYPE)
        ids = np.zeros((rows, max(pitch, 1)), np.int32)
        logp = np.zeros((rows, max(pitch, 1)), np.float32)
        first, last = np.zeros((rows, max(pitch, 1)), np.int32), np.zeros((rows, max(pitch, 1)), np.int32)
        rc = fn(self.h, *head, rows, int(window_samples), int(margin_frames), _p(info), _p(ids), _p(logp), _p(first), _p(last), pitch,
                self._stream())
        self._check(rc, what)
        return info, ids, logp, first, last

    def transcribe_windows_raw(self, log_probs, n_samples, window_samples: int = 0, margin_frames: int = -1, pitch: int | None = None):
        """qv_transcribe_windows as arrays: log_probs float32 cuda [windows of all recordings, t_max, 1025] in
        recording-then-window order, n_samples the recordings' lengths.  Returns (info [R] of LONG_INFO_DTYPE, ids int32
        [R, pitch], logp float32, first / last int32 [R, pitch])."""
        head, n, plans = self._windows_head("transcribe_windows", log_probs, n_samples, window_samples, margin_frames)
        return self._long_call(self.lib.qv_transcribe_windows, "qv_transcribe_windows", head, len(n), max(p["t_frames"] for p in plans),
                               window_samples, margin_frames, pitch)

    def _windows_head(self, what, log_probs, n_samples, window_samples, margin_frames):
        """the head arguments of a call on the caller's window log-probs, the recordings' lengths (int64) and their plans"""
        W, t_max, _ = self._logprob_args(log_probs)
        n = np.ascontiguousarray(np.asarray(n_samples, dtype=np.int64))
        plans = [self.long_plan_raw(int(v), window_samples, margin_frames) for v in n]
        if W != sum(p["n_windows"] for p in plans):
            raise QvError(f"{what}: log_probs {tuple(log_probs.shape)} does not hold the {sum(p['n_windows'] for p in plans)} planned windows")
        return (C.c_void_p(log_probs.data_ptr()), t_max, _p(n)), n, plans

    def transcribe_long_raw(self, audio, lengths, window_samples: int = 0, margin_frames: int = -1, pitch: int | None = None):
        """qv_transcribe_long as arrays (audio: float32 cuda [R, N]); see transcribe_windows_raw"""
        R, N, n = self._audio_args(audio, lengths)
        t_top = int(n.max()) // QV_LONG_HOP + 1
        head = (C.c_void_p(audio.data_ptr()), int(N), _p(n))
        return self._long_call(self.lib.qv_transcribe_long, "qv_transcribe_long", head, R, t_top, window_samples, margin_frames, pitch)

    def _long_transcripts(self, info, ids, logp, first, last) -> list[dict]:
        short = info[["n_tokens", "t_frames", "n_blank_frames", "flags", "min_token_logprob", "reserved_f", "avg_logprob",
                      "frame_avg_logprob"]]
        out = self._transcripts(short, ids, logp, first, last)
        for d, nw in zip(out, info["n_windows"].tolist()):
            d["n_windows"] = nw
        return out

    def transcribe_windows(self, log_probs, n_samples, window_s: float | None = None, margin_s: float | None = None) -> list[dict]:
        """transcribe_long behind the forward: the caller's window log-probs (transcribe_windows_raw).  Works without a model."""
        return self._long_transcripts(*self.transcribe_windows_raw(log_probs, n_samples, *self._long_args(window_s, margin_s)))

    def transcribe_long(self, audio, lengths, window_s: float | None = None, margin_s: float | None = None) -> list[dict]:
        """Greedy transcription with confidence of recordings of ANY length (float32 cuda [R, N], R <= max_batch): cut into
        overlapping windows the engine accepts, the forward over rounds of max_batch windows, of every window only the frames
        far enough from its cut edges, one collapse over the stitched sequence on the device (include/qverse.h, "recordings
        of any length").  One dict per recording as transcribe_logprobs returns it, plus "n_windows"; "first" / "last" are
        frames of the whole recording.  window_s / margin_s in seconds; None = QVERSE_LONG_WINDOW_S / QVERSE_LONG_MARGIN_S,
        else the largest window and min(50, Kw / 4) frames."""
        return self._long_transcripts(*self.transcribe_long_raw(audio, lengths, *self._long_args(window_s, margin_s)))

    # ------------------------------------------------ timings for recordings of any length -----
    def align_long_plan(self, n_samples, n_tokens, window_samples: int = 0, margin_frames: int = -1) -> dict:
        """qv_align_long_plan for this engine's max_samples; host only.  {"n_windows" (of all rows), "bytes" (the workspace a
        call with these rows would need: include/qverse.h gives the formula)}; QvError where the call would be refused."""
        n = np.ascontiguousarray(np.asarray(n_samples, dtype=np.int64).reshape(-1))
        lt = np.ascontiguousarray(np.asarray(n_tokens, dtype=np.int32).reshape(-1))
        assert len(n) == len(lt)
        nw, nbytes = C.c_int32(), C.c_int64()
        rc = self.lib.qv_align_long_plan(_p(n), _p(lt), len(n), self.max_samples,
                                         int(window_samples), int(margin_frames), C.byref(nw), C.byref(nbytes))
        if rc != 0:
            raise QvError(f"qv_align_long_plan failed ({rc}): {len(n)} rows, {int(nbytes.value)} bytes")
        return {"n_windows": int(nw.value), "bytes": int(nbytes.value)}

    def _align_long_call(self, fn, what, head, rows, targets, window_samples, margin_frames, pitch):
        assert len(targets) == rows
        lens = np.ascontiguousarray(np.array([len(x) for x in targets], np.int32))
        tg = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint16).reshape(-1) for x in targets] + [np.zeros(1, np.uint16)]))
        pitch = max(int(lens.max()), 1) if pitch is None else int(pitch)
        info = np.zeros(rows, dtype=ALIGN_LONG_INFO_DTYPE)
        first, last = np.zeros((rows, max(pitch, 1)), np.int32), np.zeros((rows, max(pitch, 1)), np.int32)
        logp = np.zeros((rows, max(pitch, 1)), np.float32)
        rc = fn(self.h, *head, rows, int(window_samples), int(margin_frames), _p(tg), _p(lens), _p(info), _p(first), _p(last), _p(logp), pitch,
                self._stream())
        self._check(rc, what)
        return info, first, last, logp

    def align_windows_raw(self, log_probs, n_samples, targets, window_samples: int = 0, margin_frames: int = -1, pitch: int | None = None):
        """qv_align_windows as arrays: log_probs float32 cuda [windows of all recordings, t_max, 1025] in recording-then-window
        order (as transcribe_windows_raw), targets a list of id lists (0..1023), one per recording.  Returns (info [R] of
        ALIGN_LONG_INFO_DTYPE, first / last int32 [R, pitch] in frames of the whole recording, logp float32 [R, pitch])."""
        head, n, _ = self._windows_head("align_windows", log_probs, n_samples, window_samples, margin_frames)
        return self._align_long_call(self.lib.qv_align_windows, "qv_align_windows", head, len(n), targets, window_samples, margin_frames, pitch)

    def align_long_raw(self, audio, lengths, targets, window_samples: int = 0, margin_frames: int = -1, pitch: int | None = None):
        """qv_align_long as arrays (audio: float32 cuda [R, N]); see align_windows_raw"""
        R, N, n = self._audio_args(audio, lengths)
        head = (C.c_void_p(audio.data_ptr()), int(N), _p(n))
        return self._align_long_call(self.lib.qv_align_long, "qv_align_long", head, R, targets, window_samples, margin_frames, pitch)

    @staticmethod
    def _long_alignments(targets, info, first, last, logp) -> list[dict]:
        out = []
        for b in range(len(info)):
            flags = int(info[b]["flags"])
            n = 0 if flags else int(info[b]["n_tokens"])
            out.append({"ids": np.asarray(targets[b], np.int32).reshape(-1)[:n], "first": first[b, :n].copy(), "last": last[b, :n].copy(),
                        "logp": logp[b, :n].copy(), "score": float(info[b]["score"]), "flags": flags,
                        "n_tokens": int(info[b]["n_tokens"]), "t_frames": int(info[b]["t_frames"]), "n_windows": int(info[b]["n_windows"])})
        return out

    def align_windows(self, log_probs, n_samples, targets, window_s: float | None = None, margin_s: float | None = None) -> list[dict]:
        """align_long behind the forward: the caller's window log-probs (align_windows_raw).  Works without a model."""
        return self._long_alignments(targets, *self.align_windows_raw(log_probs, n_samples, targets, *self._long_args(window_s, margin_s)))

    def align_long(self, audio, lengths, targets, window_s: float | None = None, margin_s: float | None = None) -> list[dict]:
        """CTC forced alignment of token lists of up to 16,383 ids against recordings of ANY length (float32 cuda [R, N],
        R <= max_batch): the windows and rounds of transcribe_long, every window's owned log-prob rows kept at their frame of
        the whole recording, one Viterbi pass per recording on the device (include/qverse.h, "word and verse timings for
        recordings of any length").  One dict per recording as align() returns it -- "ids", "first", "last" (frames of the whole
        recording, 0.08 s each), "logp", "score", "flags", "n_tokens", "t_frames" -- plus "n_windows"."""
        return self._long_alignments(targets, *self.align_long_raw(audio, lengths, targets, *self._long_args(window_s, margin_s)))

    def align_long_kernel_times(self) -> dict:
        """milliseconds the last align_long / align_windows call spent in its own two kernels (HIP events; needs
        profile_stages(True))"""
        ms = (C.c_float * 2)()
        self._check(self.lib.qv_align_long_kernel_times(self.h, ms), "qv_align_long_kernel_times")
        return {"keep": ms[0], "align": ms[1]}

    def long_kernel_times(self) -> dict:
        """milliseconds the last transcribe_long / transcribe_windows call spent in its own three kernels (HIP events; needs
        profile_stages(True))"""
        ms = (C.c_float * 3)()
        self._check(self.lib.qv_long_kernel_times(self.h, ms), "qv_long_kernel_times")
        return {"gather": ms[0], "frames": ms[1], "collapse": ms[2]}

    def debug_retrieve(self, transcript: str) -> dict:
        """match_verse + candidate assembly for an already-normalised transcript."""
        codes = np.ascontiguousarray(self.tables.encode(transcript))
        cap = 2048
        bs, bp, nc, nr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        bsc = C.c_double()
        cs = np.zeros(cap, np.int32)
        cp = np.zeros(cap, np.int32)
        csc = np.zeros(cap, np.float64)
        ri = np.zeros(128, np.int32)
        rs = np.zeros(128, np.float64)
        rc = self.lib.qv_debug_retrieve(self.h, _p(codes), len(codes), C.byref(bs), C.byref(bp), C.byref(bsc),
                                        _p(cs), _p(cp), _p(csc), cap, C.byref(nc), _p(ri), _p(rs), C.byref(nr),
                                        self._stream())
        self._check(rc, "qv_debug_retrieve")
        n = min(nc.value, cap)
        return {"base_start": bs.value, "base_span": bp.value, "base_score": bsc.value,
                "cand_start": cs[:n].copy(), "cand_span": cp[:n].copy(), "cand_score": csc[:n].copy(),
                "runner_idx": ri[: nr.value].copy(), "runner_score": rs[: nr.value].copy()}

    def transcript_codes(self, ctx: int | None = None, batch: int = 1) -> list[dict]:
        """The normalised transcript the decode kernel left on the device for every row of context `ctx`'s last batch
        (default: the most recent call's) -- the codes the matching kernels read (qv_debug_transcript_codes).  Per row
        {"codes": uint8 array (tables.encode of the transcript), "n_chars", "n_words"}; a row flagged EMPTY or TRUNCATED
        has no codes.  Call it before the context is reused."""
        if ctx is None:
            ctx = int(self.lib.qv_last_context(self.h))
        pitch = self.max_transcript
        codes = np.zeros((batch, pitch), np.uint8)
        n, words = np.zeros(batch, np.int32), np.zeros(batch, np.int32)
        rc = self.lib.qv_debug_transcript_codes(self.h, int(ctx), int(batch), _p(codes), pitch, _p(n), _p(words))
        self._check(rc, "qv_debug_transcript_codes")
        return [{"codes": codes[b, : n[b]].copy(), "n_chars": int(n[b]), "n_words": int(words[b])} for b in range(batch)]

    def debug_ctc_loss(self, log_probs_2d, id_lists) -> np.ndarray:
        assert log_probs_2d.is_cuda and log_probs_2d.dim() == 2 and log_probs_2d.is_contiguous()
        tg = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint16) for x in id_lists]))
        lens = np.ascontiguousarray(np.array([len(x) for x in id_lists], np.int32))
        out = np.zeros(len(id_lists), np.float32)
        rc = self.lib.qv_debug_ctc_loss(self.h, C.c_void_p(log_probs_2d.data_ptr()), log_probs_2d.shape[0],
                                        _p(tg), _p(lens), len(id_lists), _p(out), self._stream())
        self._check(rc, "qv_debug_ctc_loss")
        return out

    TAP_C1 = 11   # forward_tap code: conv.2 output of the f16 front end (k_sub01's own result), f32[B, t2_max, 20, 256]

    def sub01_plan(self, n_samples: int, batch: int = 1) -> dict:
        """the forward's own frame arithmetic for a clip of n_samples (qv_debug_sub01_plan): frames after the log-mel front
        end and after conv.0 / conv.2 / conv.5, and the tiles of four conv.2 frames a block of the fused subsampling kernel
        walks when `batch` clips, the longest of n_samples, are launched."""
        fr, run = (C.c_int32 * 4)(), C.c_int32(0)
        self._check(self.lib.qv_debug_sub01_plan(int(n_samples), int(batch), fr, C.byref(run)), "qv_debug_sub01_plan")
        return {"mel": fr[0], "c0": fr[1], "c1": fr[2], "frames": fr[3], "run_tiles": run.value}

    TAP_C2 = 12   # forward_tap code: conv.5 output of the f16 front end, dense f32[B, t3_max, 10, 256], frames >= len3[b] zero

    def sub35_plan(self, n_samples: int, batch: int = 1) -> dict:
        """conv.5 frames one block of the fused conv.3 + conv.5 kernel walks when `batch` clips, the longest of n_samples,
        are launched (qv_debug_sub35_plan; kernel_variant(6, .) forces 1 step, 2 steps or the maximum)."""
        run = C.c_int32(0)
        self._check(self.lib.qv_debug_sub35_plan(int(n_samples), int(batch), C.byref(run)), "qv_debug_sub35_plan")
        return {"run_frames": run.value}

    def forward_tap(self, what: int, layer: int, shape=None, c1_frames: int | None = None, batch: int | None = None):
        """a tensor of the last forward as f32 (qv_debug_forward_tap).  what = TAP_C1 needs no `shape`: give the batch size
        and the longest clip's conv.2 frame count (sub01_plan(...)["c1"])."""
        if shape is None:
            assert what == self.TAP_C1 and c1_frames and batch, "only the c1 tap derives its shape"
            shape = (batch, c1_frames, 20, 256)
        out = self.torch.empty(shape, dtype=self.torch.float32, device=f"cuda:{self.device}")
        rc = self.lib.qv_debug_forward_tap(self.h, what, layer, C.c_void_p(out.data_ptr()), self._stream())
        self._check(rc, "qv_debug_forward_tap")
        return out


_hip = None


def _hip_runtime():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return _hip
