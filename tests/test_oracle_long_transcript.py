"""Transcripts of more than 1,024 normalised characters, the parts that need no GPU: the CPU oracle (no length limit)
reproduces the reference's own answers in that regime -- which is what lets the GPU tests of the wide matching window
(tests/test_gpu_long_transcript.py) lean on it -- plus the host-side pieces of the window option: front_window at 2,048,
the appended qv_config field and the struct_size rule of qv_create."""

import ctypes as C
import json

import pytest


@pytest.fixture(scope="module")
def long_cases(golden_dir):
    cases = json.loads((golden_dir / "longtx_cases.json").read_text(encoding="utf-8"))
    assert [c["chars"] for c in cases] == [1378, 1556]
    return cases


def test_oracle_reproduces_the_reference_on_transcripts_beyond_1024_characters(oracle, long_cases):
    """StreamingPipeline.run_on_full_transcript over MatchVerseOracle.match_verse (CPU, any length) against the reference's
    own run on 1,378 and 1,556 characters (tests/golden/gen_longtx_golden.py): the whole emission lists, scores included."""
    from offline_tarteel_amd.streaming import StreamingPipeline
    from oracle.tracker_ref import MatchVerseOracle

    mv = MatchVerseOracle(oracle)
    pipe = StreamingPipeline(match_verse_fn=lambda text, max_span, hint: mv.match_verse(text, max_span=max_span, hint=hint))
    for c in long_cases:
        assert pipe.run_on_full_transcript("x.wav", lambda p, t=c["text"]: t) == c["emissions"], c["chars"]
    assert [(e["surah"], e["ayah"]) for e in long_cases[0]["emissions"]] == [(2, a) for a in range(282, 287)]
    assert len(long_cases[1]["emissions"]) == 13 and long_cases[1]["emissions"][0]["ayah"] == 244


def test_front_window_at_the_wide_limit(long_cases):
    from offline_tarteel_amd.engine import QV_MAX_TRANSCRIPT, QV_MAX_TRANSCRIPT_WIDE, front_window

    assert (QV_MAX_TRANSCRIPT, QV_MAX_TRANSCRIPT_WIDE) == (1024, 2048)
    for c in long_cases:                                       # fits the wide window whole, is cut by the default one
        assert front_window(c["text"], 2048) == c["text"]
        assert len(front_window(c["text"])) <= 1024 and front_window(c["text"]) == front_window(c["text"], 1024)
    text = " ".join([long_cases[0]["text"]] * 2)               # 2,757 characters
    win = front_window(text, 2048)
    assert len(win) <= 2048 and text.startswith(win) and text[len(win)] == " " and not win.endswith(" ")
    assert len(front_window(text, 2048)) > 2048 - 20           # the LONGEST whole-word prefix (words here are short)
    assert front_window("ا" * 2048, 2048) == "ا" * 2048
    assert front_window("ا" * 2049, 2048) == "ا" * 2048       # no space to cut at: a hard cut
    exact = ("ا" * 2048) + " " + "ب"
    assert front_window(exact, 2048) == "ا" * 2048             # the space right behind the window counts


def _lib():
    from offline_tarteel_amd.engine import load_library

    return load_library()


def test_config_default_and_the_abi_stub_carry_the_window_field():
    from offline_tarteel_amd.engine import QvConfig

    lib = _lib()
    assert QvConfig._fields_[-1] == ("max_transcript", C.c_int32)
    assert [n for n, _ in QvConfig._fields_][-2] == "n_contexts"     # appended: everything in front keeps its offset
    cfg = QvConfig()
    lib.qv_config_default(C.byref(cfg))
    assert cfg.max_transcript == 1024 and cfg.struct_size == C.sizeof(QvConfig)
    assert hasattr(lib, "qv_max_transcript")
    lib.qv_max_transcript.argtypes = [C.c_void_p]
    assert lib.qv_max_transcript(None) == 0


def test_qv_create_accepts_the_first_layout_and_checks_the_window():
    """struct_size of the layout that ends with n_contexts is an older caller (window field read as 0 = 1,024): it gets past
    the argument checks -- to "no HIP device" on a box without a GPU, to a working engine with one.  A struct_size that is
    neither, and a window other than 0 / 1024 / 2048, are argument errors with a message."""
    from offline_tarteel_amd import TABLES_PATH
    from offline_tarteel_amd.engine import QvConfig

    lib = _lib()
    lib.qv_last_error.argtypes = [C.c_void_p]
    lib.qv_last_error.restype = C.c_char_p
    lib.qv_max_transcript.argtypes = [C.c_void_p]
    lib.qv_destroy.argtypes = [C.c_void_p]
    lib.qv_destroy.restype = None
    tables = str(TABLES_PATH).encode()

    def create(struct_size=None, window=None):
        cfg = QvConfig()
        lib.qv_config_default(C.byref(cfg))
        cfg.tables_path, cfg.with_model, cfg.max_batch = tables, 0, 1
        if window is not None:
            cfg.max_transcript = window
        if struct_size is not None:
            cfg.struct_size = struct_size
            cfg.max_transcript = 777          # behind an old caller's struct: must not be read
        h = C.c_void_p()
        rc = lib.qv_create(C.byref(cfg), C.byref(h))
        msg = lib.qv_last_error(None).decode() if rc else ""
        got = lib.qv_max_transcript(h) if rc == 0 else None
        if rc == 0:
            lib.qv_destroy(h)
        return rc, msg, got

    old = QvConfig.n_contexts.offset + 4
    assert old < C.sizeof(QvConfig)
    rc, msg, got = create(struct_size=old)
    assert rc in (0, 3) and "struct_size" not in msg and "max_transcript" not in msg, (rc, msg)   # 3 = QV_ERR_HIP: no device
    assert got in (None, 1024)
    for bad in (old - 4, C.sizeof(QvConfig) + 8, 0):
        rc, msg, _ = create(struct_size=bad)
        assert rc == 1 and "struct_size" in msg, (bad, rc, msg)
    for window in (1, 1023, 1536, 4096, -1):
        rc, msg, _ = create(window=window)
        assert rc == 1 and "max_transcript" in msg, (window, rc, msg)
    for window, want in ((0, 1024), (1024, 1024), (2048, 2048)):
        rc, msg, got = create(window=window)
        assert rc in (0, 3) and "max_transcript" not in msg, (window, rc, msg)
        assert got in (None, want)
