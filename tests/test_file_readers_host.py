"""The two file readers behind qv_create (csrc/qv_tables_host.h: the tables file -> every host array the engine uploads;
csrc/qv_weights_host.h: the weight file) are pure host logic.  tools/file_readers_check.cpp is built here with the host
compiler under AddressSanitizer + UBSan and run as a plain executable: on the committed tables file every derived array must
equal a numpy recomputation from the documented layouts (csrc/qv_common.h: QvTables, tools/build_tables.py), and every
malformed file must be refused with a message -- not crash, not trip a sanitizer, not be accepted."""
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tables_patch import MALFORMED, QV_MAX_SPAN, QV_VOCAB, TABLES, TablesFile, malformed

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "offline-tarteel_amd" / "csrc"
QV_NSYM = 40
REFUSED = 3


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    src = ROOT / "tools" / "file_readers_check.cpp"
    for f in (src, CSRC / "qv_tables_host.h", CSRC / "qv_weights_host.h", CSRC / "qv_limits.h"):   # and no HIP behind them
        assert not any("hip" in inc for inc in re.findall(r'#include\s*[<"]([^>"]+)[>"]', f.read_text())), f
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("file_readers") / "file_readers_check"
    # the sanitizer runtimes are linked INTO the executable, so it runs in whatever environment the suite runs in
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         *static_rt, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr

    def run(*args):
        # an allocation sized from an unchecked count in a file is an error here, not a 16 GB reservation
        env = dict(os.environ, ASAN_OPTIONS="max_allocation_size_mb=1024:allocator_may_return_null=0")
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120, env=env)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
        return p

    return run


def refused_with(p, names):
    assert p.returncode == REFUSED, (p.returncode, p.stdout, p.stderr)
    m = re.match(r"refused: (.+)", p.stdout)
    assert m and names in m.group(1), p.stdout
    return m.group(1)


# ---------------------------------------------------------------- the committed tables file ----
def tmpl_w(words):
    """word counts the LCS core is instantiated for (qv_tmpl_w)"""
    return next(w for w in (1, 2, 3, 4, 6, 8, 11, 16) if words <= w or w == 16)


def match_masks(codes):
    """[QV_NSYM][qv_tmpl_w(ceil(len / 64))] u64: bit i of row c is set where code i of the text is c"""
    m = np.zeros((QV_NSYM, tmpl_w((len(codes) + 63) // 64)), np.uint64)
    i = np.flatnonzero(codes < QV_NSYM)
    np.bitwise_or.at(m, (codes[i], i >> 6), np.uint64(1) << (i & 63).astype(np.uint64))
    return m


def expected_arrays():
    f = TablesFile()
    s = {k: f.sec(k) for k in f.dir if k in ("meta", "clean_off", "clean", "alt_off", "alt", "nobsm_off", "nobsm", "tok_off", "tok",
                                             "piece_off", "piece_codes", "tri_keys", "vtri_off", "vtri")}
    N, NT = int(s["meta"][0]), int(s["meta"][6])
    text = lambda name, v: s[name][s[name + "_off"][v]:s[name + "_off"][v + 1]]   # noqa: E731
    clean = [text("clean", v) for v in range(N)]
    clen, alen, nlen = (np.diff(s[k + "_off"][:N + 1].astype(np.int64)) for k in ("clean", "alt", "nobsm"))
    e = {}
    # clean: the texts back to back with one ' ' (code 0) behind each, 64 bytes of 0 at the end
    e["clean"] = np.concatenate([np.append(c, np.uint8(0)) for c in clean] + [np.zeros(64, np.uint8)])
    e["clean_off"] = (np.cumsum(clen + 1) - (clen + 1)).astype(np.uint32)
    e["clean_len"], e["alt_len"], e["nobsm_len"] = clen.astype(np.uint16), alen.astype(np.uint16), nlen.astype(np.uint16)
    # clean8: per verse one ' ', its codes, 0xFF up to a multiple of 8; 64 bytes of 0xFF at the end
    blocks = [np.concatenate([[0], c, np.full(-(len(c) + 1) % 8, 0xFF)]).astype(np.uint8) for c in clean]
    e["clean8"] = np.concatenate(blocks + [np.full(64, 0xFF, np.uint8)])
    e["clean8_off"] = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint32)
    e["alt"] = np.concatenate([s["alt"][:s["alt_off"][N]], np.zeros(64, np.uint8)])
    e["alt_off"] = s["alt_off"][:N].astype(np.uint32)
    has = nlen > 0
    e["nobsm_rank"] = np.where(has, np.cumsum(has) - 1, -1).astype(np.int32)
    # wend: chars of the first k + 1 words joined = positions of the spaces, then the length
    wends = [np.append(np.flatnonzero(c == 0), len(c)) for c in clean]
    e["wend"] = np.concatenate(wends).astype(np.uint16)
    e["wend_off"] = np.concatenate([[0], np.cumsum([len(w) for w in wends])]).astype(np.uint32)
    e["len_order"] = np.argsort(-clen, kind="stable").astype(np.int32)
    # pmv: text id = variant * N + v for clean / alt, 2N + nobsm_rank for the no-bismillah texts; 16 words of 0 at the end
    masks = [match_masks(c) for c in clean] + [match_masks(text("alt", v)) for v in range(N)] + \
            [match_masks(text("nobsm", v)) for v in np.flatnonzero(has)]
    e["pmv"] = np.concatenate([m.ravel() for m in masks] + [np.zeros(16, np.uint64)])
    sizes = np.array([m.size for m in masks])
    e["pmv_off"] = (np.cumsum(sizes) - sizes).astype(np.uint32)
    # inverted trigram index: the verses of each trigram in ascending order; 64 entries of 0 at the end
    verse_of = np.repeat(np.arange(N), np.diff(s["vtri_off"][:N + 1].astype(np.int64)))
    ids = s["vtri"][:s["vtri_off"][N]].astype(np.int64)
    by_id = np.argsort(ids, kind="stable")
    e["tri_post"] = np.concatenate([verse_of[by_id], np.zeros(64, np.int64)]).astype(np.uint16)
    start = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=NT))])
    # tri_slice[id][w]: where the verses of quarter w of the verse range start in the trigram's list (w = 4: its end)
    quarters = [start[:-1] + np.bincount(ids[verse_of < w * N // 4], minlength=NT) for w in range(4)] + [start[1:]]
    e["tri_slice"] = np.stack(quarters, axis=1).astype(np.uint32).ravel()
    e["tri_map"] = np.full(1 << 18, 0xFFFF, np.uint16)
    e["tri_map"][s["tri_keys"][:NT]] = np.arange(NT)
    # tok_pfx: bit k - 1 set where the ids of (v, span k) are a non-empty prefix of the ids of (v, span k + 1)
    to, tok, pfx = s["tok_off"].astype(np.int64), s["tok"], np.zeros(N, np.uint8)
    for v in range(N):
        for k in range(1, QV_MAX_SPAN):
            a0, a1, b1 = to[v * QV_MAX_SPAN + k - 1:v * QV_MAX_SPAN + k + 2]
            if a1 > a0 and b1 - a1 >= a1 - a0 and np.array_equal(tok[a0:a1], tok[a1:a1 + (a1 - a0)]):
                pfx[v] |= 1 << (k - 1)
    e["tok_pfx"] = pfx
    e["piece_codes"] = np.concatenate([s["piece_codes"][:s["piece_off"][QV_VOCAB]], np.zeros(16, np.uint8)])
    return e, (N, int(s["meta"][1]), NT, 2 * N + int(has.sum()))


def test_committed_tables_derive_what_the_layouts_say(checker, tmp_path):
    p = checker("tables", TABLES, "--dump", tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    want, counts = expected_arrays()
    assert p.stdout.strip() == "tables ok: n_verses %d n_surah %d n_tri %d n_text %d" % counts
    assert len(want) == 20 and sorted(want) == sorted(x.name for x in tmp_path.iterdir())
    for name, w in want.items():
        got = np.fromfile(tmp_path / name, dtype=w.dtype)
        assert got.shape == w.shape and np.array_equal(got, w), name


# ---------------------------------------------------------------- malformed tables ----
@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_tables_are_refused(checker, tmp_path, case):
    msg = refused_with(checker("tables", malformed(case, tmp_path / "tables.bin")), MALFORMED[case][1])
    print(case, "->", msg)


def test_a_tables_path_that_does_not_exist_is_refused(checker, tmp_path):
    """the reader every caller shares (qv_read_host_tables): qv_create's message, with the path"""
    missing = tmp_path / "no_such_tables.bin"
    assert refused_with(checker("tables", missing), "cannot open tables file:") == f"cannot open tables file: {missing}"


def test_an_empty_tables_file_is_refused_by_the_bad_magic_rule(checker, tmp_path):
    (tmp_path / "tables.bin").write_bytes(b"")
    p = checker("tables", tmp_path / "tables.bin")
    assert refused_with(p, "bad magic") == "tables file malformed (bad magic)"
    # ... the message a file with another magic gets, not one of its own
    (tmp_path / "other.bin").write_bytes(b"QVTB0002" + bytes(64))
    assert checker("tables", tmp_path / "other.bin").stdout == p.stdout


# ---------------------------------------------------------------- malformed weights ----
def tensor(name: bytes, numel: int, data: bytes | None = None) -> bytes:
    return struct.pack("<I", len(name)) + name + struct.pack("<I", numel) + (bytes(4 * numel) if data is None else data)


WEIGHT_FILES = {
    "bad_magic": (b"QVWT0002" + struct.pack("<I", 0), "magic"),
    "cut_inside_the_header": (b"QVWT0001\x01\x00", "magic"),
    "name_length_513": (b"QVWT0001" + struct.pack("<II", 1, 513) + bytes(600), "malformed"),
    "numel_exceeds_the_file": ((b"QVWT0001" + struct.pack("<I", 1) + tensor(b"a", 0xFFFFFFFF, b"")).ljust(64, b"\0"), "truncated"),
    "count_ffffffff_one_tensor": (b"QVWT0001" + struct.pack("<I", 0xFFFFFFFF) + tensor(b"a", 1), "tensors do not fit"),
    "one_tensor_only": (b"QVWT0001" + struct.pack("<I", 1) + tensor(b"some.tensor", 3), "lacks tensor"),
}


@pytest.mark.parametrize("case", list(WEIGHT_FILES))
def test_malformed_weight_files_are_refused(checker, tmp_path, case):
    data, names = WEIGHT_FILES[case]
    (tmp_path / "weights.bin").write_bytes(data)
    refused_with(checker("weights", tmp_path / "weights.bin"), names)
