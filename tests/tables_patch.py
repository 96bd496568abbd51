"""Malformed copies of the committed tables file, made by patching its bytes (tests/test_file_readers_host.py, and the
engine-creation tests of tests/test_gpu_postlogits.py).  Layout: tools/build_tables.py."""
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
TABLES = ROOT / "offline-tarteel_amd" / "data" / "qverse_tables.bin"
QV_VOCAB, QV_MAX_SPAN, QV_MAX_VW = 1025, 6, 11
MAX_TEXT = 64 * QV_MAX_VW

DTYPES = {"meta": "<i4", "surah": "u1", "ayah": "<u2", "surah_start": "<i4", "surah_len": "<i4", "clean_off": "<u4", "clean": "u1",
          "alt_off": "<u4", "alt": "u1", "nobsm_off": "<u4", "nobsm": "u1", "clean_nw": "<u2", "alt_nw": "<u2", "nobsm_nw": "<u2",
          "tok_off": "<u4", "tok": "<u2", "piece_off": "<u4", "piece_codes": "u1", "tri_keys": "<u4", "tri_idf": "<f8",
          "vtri_off": "<u4", "vtri": "<u2"}


class TablesFile:
    """The file's bytes (mutable) with its directory: name -> (entry index, offset, nbytes)."""

    def __init__(self, data: bytes | None = None):
        self.b = bytearray(TABLES.read_bytes() if data is None else data)
        assert self.b[:8] == b"QVTB0001"
        self.n_sec = struct.unpack_from("<I", self.b, 8)[0]
        self.dir = {}
        for i in range(self.n_sec):
            e = 16 + 40 * i
            name = bytes(self.b[e:e + 24]).rstrip(b"\0").decode()
            self.dir[name] = (i, *struct.unpack_from("<QQ", self.b, e + 24))

    def sec(self, name) -> np.ndarray:
        """a writable view of the section's elements"""
        _, off, nb = self.dir[name]
        return np.frombuffer(self.b, dtype=DTYPES[name], count=nb // np.dtype(DTYPES[name]).itemsize, offset=off)

    def set_entry(self, name, off=None, nb=None, rename=None):
        i, o, n = self.dir[name]
        e = 16 + 40 * i
        if rename is not None:
            self.b[e:e + 24] = rename.encode().ljust(24, b"\0")
        struct.pack_into("<QQ", self.b, e + 24, o if off is None else off, n if nb is None else nb)

    def write(self, path) -> Path:
        Path(path).write_bytes(self.b)
        return Path(path)


def _cut(n):
    return lambda f: f.b.__delitem__(slice(n(f), None))


def _meta0(value):
    def patch(f):
        f.sec("meta")[0] = value(f) if callable(value) else value
    return patch


def _entry(name, **kw):
    return lambda f: f.set_entry(name, **{k: (v(f) if callable(v) else v) for k, v in kw.items()})


def _last_off(off_name, into):
    def patch(f):
        f.sec(off_name)[-1] = len(f.sec(into)) + 1   # (every offset section of the file holds exactly its n + 1 entries)
    return patch


def _swap_clean_off(f):
    o = f.sec("clean_off")
    assert o[10] != o[11]
    o[10], o[11] = int(o[11]), int(o[10])


def _overlong_verse(f):
    o = f.sec("clean_off")
    k = int(np.searchsorted(o, int(o[0]) + MAX_TEXT, side="right")) - 1   # o[k + 1] is the first end past the limit
    assert o[k + 1] - o[0] > MAX_TEXT >= o[k] - o[0]
    o[1:k + 1] = o[k + 1]


def _set(name, index, value):
    def patch(f):
        f.sec(name)[index] = value(f) if callable(value) else value
    return patch


def _nobsm_byte(f):
    f.sec("nobsm")[0] ^= 1   # the first code of the first no-bismillah text


def _n(f):
    return int(f.sec("meta")[0])


# case -> (patch, what the message must name)
MALFORMED = {
    "cut_to_12_bytes": (_cut(lambda f: 12), "magic"),
    "directory_one_byte_short": (_cut(lambda f: 16 + 40 * f.n_sec - 1), "directory"),
    "section_count_ffffffff": (lambda f: struct.pack_into("<I", f.b, 8, 0xFFFFFFFF), "directory"),
    "entry_offset_wraps": (_entry("ayah", off=2 ** 64 - 8, nb=16), "ayah"),
    "required_section_renamed": (_entry("tok", rename="tok_gone"), "lacks section tok"),
    "meta_8_bytes": (_entry("meta", nb=8), "meta"),
    "meta0_n_plus_1": (_meta0(lambda f: _n(f) + 1), "section"),
    "meta0_minus_1": (_meta0(-1), "meta"),
    "meta0_70000": (_meta0(70000), "meta"),
    "ayah_halved": (_entry("ayah", nb=lambda f: f.dir["ayah"][2] // 2), "ayah"),
    "clean_off_end_past_clean": (_last_off("clean_off", "clean"), "clean_off"),
    "clean_off_neighbours_swapped": (_swap_clean_off, "clean_off"),
    "verse_0_over_the_text_limit": (_overlong_verse, "clean"),
    "vtri_off_end_past_vtri": (_last_off("vtri_off", "vtri"), "vtri_off"),
    "vtri_id_is_n_tri": (_set("vtri", 0, lambda f: int(f.sec("meta")[6])), "vtri"),
    "tri_key_2_18": (_set("tri_keys", 0, 1 << 18), "tri_keys"),
    "tok_off_end_past_tok": (_last_off("tok_off", "tok"), "tok_off"),
    "tok_id_is_vocab": (_set("tok", 5, QV_VOCAB), "tok"),
    "piece_off_end_past_piece_codes": (_last_off("piece_off", "piece_codes"), "piece_off"),
    "nobsm_byte_changed": (_nobsm_byte, "no_bsm"),
}


def malformed(case, path) -> Path:
    f = TablesFile()
    MALFORMED[case][0](f)
    return f.write(path)
