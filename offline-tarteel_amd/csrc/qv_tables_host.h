// qv_tables_host.h -- qverse_tables.bin on the host: parse, validate, derive.  HIP-free (the standard library only), so
// tools/file_readers_check.cpp runs it under ASan + UBSan on a machine without a GPU; qv_capi.hip uploads the result.
//
// File layout (tools/build_tables.py): "QVTB0001", u32 n_sections, u32 0, n x {char name[24]; u64 offset; u64 nbytes},
// then the payloads.  The file is NOT trusted: every value that is later used as a count, an offset or an index -- here
// or in a kernel -- is checked against the size of what it indexes before anything is derived from it.
//
// What the kernels assume about the content, and where:
//   n_verses <= QV_MAX_VERSES    k_lcs_full packs a work item as utterance << 15 | verse << 2 | variant and k_frag takes
//                                13 bits of verse back out (qv_match_body.inc); tri_post holds verses as uint16_t
//   n_tri < 0xFFFF               tri_map holds trigram ids as uint16_t, 0xFFFF = not in the index
//   tri_keys < 2^18              three 6-bit codes; tri_map has 2^18 entries
//   text length <= QV_MAX_TEXT   = 64 * QV_MAX_VW codes, all three texts of a verse (text_of hands any of them out).  A verse
//                                text is the PATTERN of an LCS in k_frag (transcript longer than the text) and k_hint_sp:
//                                both dispatch with WMAX = QV_MAX_VW words, k_frag copies the masks into an LDS slice of
//                                FRAG_PM_STRIDE words per symbol, and the mask rows built here are qv_tmpl_w(words) wide,
//                                which stops growing at 16 words.  The longest text of the committed file is 678 codes.
//   tok ids < QV_VOCAB           they index log-prob columns (CTC rerank, forced alignment)
//   vtri ids < n_tri             they index tri_idf on the device and the inverted index built here
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <type_traits>
#include <vector>

#include "qv_limits.h"

#define QV_MAX_VERSES 8192
#define QV_MAX_TEXT (64 * QV_MAX_VW)

// a section that is uploaded as it stands: a view into the file's bytes (valid while the caller keeps them)
template <typename T>
struct QvView {
    const T *p = nullptr;
    size_t n = 0;
    const T *data() const { return p; }
    size_t size() const { return n; }
    const T &operator[](size_t i) const { return p[i]; }
};

// the largest element: a pass without an exit, so it vectorises (tok alone has 3.7 M entries)
template <typename T>
inline T qv_largest(const T *p, size_t n) {
    T m = 0;
    for (size_t i = 0; i < n; ++i) m = p[i] > m ? p[i] : m;
    return m;
}

// Everything QvTables (qv_common.h) points at, on the host, under the same names and in the same layouts.
struct HostTables {
    int n_verses = 0, n_surah = 0, n_tri = 0, n_text = 0;
    QvView<uint8_t> surah;
    QvView<uint16_t> ayah;
    QvView<int32_t> surah_start, surah_len;
    std::vector<uint8_t> clean;
    std::vector<uint32_t> clean_off;
    std::vector<uint16_t> clean_len, nobsm_len;
    std::vector<uint8_t> clean8;
    std::vector<uint32_t> clean8_off;
    std::vector<uint8_t> alt;
    std::vector<uint32_t> alt_off;
    std::vector<uint16_t> alt_len;
    QvView<uint16_t> nw[3];
    std::vector<int32_t> nobsm_rank;
    std::vector<uint32_t> wend_off;
    std::vector<uint16_t> wend;
    std::vector<int32_t> len_order;
    std::vector<uint64_t> pmv;
    std::vector<uint32_t> pmv_off;
    QvView<uint32_t> tri_keys;
    QvView<double> tri_idf;
    QvView<uint32_t> vtri_off;
    QvView<uint16_t> vtri;
    std::vector<uint16_t> tri_post, tri_map;
    std::vector<uint32_t> tri_slice;
    QvView<uint32_t> tok_off;
    QvView<uint16_t> tok;
    std::vector<uint8_t> tok_pfx;
    QvView<uint32_t> piece_off;
    std::vector<uint8_t> piece_codes;
    // host copies the engine keeps
    std::vector<uint8_t> h_surah;
    std::vector<uint16_t> h_ayah;
    std::vector<uint8_t> file;   // qv_read_host_tables: the file's bytes, which the views point into
};

// `data` must be aligned for uint64_t (a std::vector's or malloc's storage is) and outlive `out`, whose views point into it.
inline int qv_build_host_tables(const uint8_t *data, size_t size, HostTables &out, std::string &err) {
    auto fail = [&](const std::string &msg) { err = msg; return (int)QV_ERR_IO; };
    if (size < 16 || memcmp(data, "QVTB0001", 8)) return fail("tables file malformed (bad magic)");
    uint32_t n_sec;
    memcpy(&n_sec, data + 8, 4);
    if (n_sec > (size - 16) / 40) return fail("tables file malformed (directory of " + std::to_string(n_sec) + " sections exceeds the file)");
    // section `name` as `count` elements of T at least; false with `err` set otherwise
    auto section = [&](const char *name, size_t count, auto &view) -> bool {
        using T = typename std::remove_reference<decltype(*view.p)>::type;
        for (uint32_t i = 0; i < n_sec; ++i) {
            const uint8_t *e = data + 16 + 40 * (size_t)i;
            if (strncmp((const char *)e, name, 24) != 0) continue;
            uint64_t off, nb;
            memcpy(&off, e + 24, 8);
            memcpy(&nb, e + 32, 8);
            if (off > size || nb > size - off || off % 8 != 0) { err = std::string("tables: section ") + name + " lies outside the file or is misaligned"; return false; }
            if (nb / sizeof(T) < count) {
                err = std::string("tables: section ") + name + " holds " + std::to_string(nb) + " bytes, " + std::to_string(count) + " x " + std::to_string(sizeof(T)) + " needed";
                return false;
            }
            view.p = (const T *)(data + off);
            view.n = (size_t)(nb / sizeof(T));
            return true;
        }
        err = std::string("tables file lacks section ") + name;
        return false;
    };
    // offsets `off` [0 .. n]: non-decreasing, the last one inside the `limit` elements of section `into`
    auto offsets_ok = [&](const char *name, const QvView<uint32_t> &off, size_t n, const char *into, size_t limit) -> bool {
        for (size_t i = 0; i < n; ++i)
            if (off[i] > off[i + 1]) { err = std::string("tables: ") + name + " decreases at entry " + std::to_string(i + 1); return false; }
        if (off[n] > limit) { err = std::string("tables: ") + name + " ends past section " + into; return false; }
        return true;
    };

    QvView<int32_t> meta;
    if (!section("meta", 7, meta)) return QV_ERR_IO;
    const int N = meta[0], NS = meta[1], K = meta[2], NT = meta[6];
    if (K > QV_NSYM || meta[3] != QV_MAX_SPAN || meta[4] != QV_VOCAB) return fail("tables file incompatible (alphabet/max_span/vocab)");
    if (N <= 0 || N > 65535 || N > QV_MAX_VERSES) return fail("tables: meta gives " + std::to_string(N) + " verses (1 .. " + std::to_string(QV_MAX_VERSES) + ")");
    if (NS <= 0 || NS > N) return fail("tables: meta gives " + std::to_string(NS) + " surahs");
    if (NT < 0 || NT >= 0xFFFF) return fail("tables: meta gives " + std::to_string(NT) + " trigrams (tri_keys: trigram key out of range)");
    const size_t Nz = (size_t)N, NK = Nz * QV_MAX_SPAN;

    HostTables &t = out;
    t = HostTables();
    t.n_verses = N; t.n_surah = NS; t.n_tri = NT;
    QvView<uint32_t> coff, aoff, noff;
    QvView<uint8_t> ctxt, atxt, ntxt, pcodes;
    if (!section("surah", Nz, t.surah) || !section("ayah", Nz, t.ayah) || !section("surah_start", (size_t)NS + 1, t.surah_start) ||
        !section("surah_len", (size_t)NS, t.surah_len) || !section("clean_off", Nz + 1, coff) || !section("clean", 0, ctxt) ||
        !section("alt_off", Nz + 1, aoff) || !section("alt", 0, atxt) || !section("nobsm_off", Nz + 1, noff) ||
        !section("nobsm", 0, ntxt) || !section("clean_nw", Nz, t.nw[0]) || !section("alt_nw", Nz, t.nw[1]) ||
        !section("nobsm_nw", Nz, t.nw[2]) || !section("tok_off", NK + 1, t.tok_off) || !section("tok", 0, t.tok) ||
        !section("piece_off", (size_t)QV_VOCAB + 1, t.piece_off) || !section("piece_codes", 0, pcodes) ||
        !section("tri_keys", (size_t)NT, t.tri_keys) || !section("tri_idf", (size_t)NT, t.tri_idf) ||
        !section("vtri_off", Nz + 1, t.vtri_off) || !section("vtri", 0, t.vtri))
        return QV_ERR_IO;
    if (!offsets_ok("clean_off", coff, Nz, "clean", ctxt.n) || !offsets_ok("alt_off", aoff, Nz, "alt", atxt.n) ||
        !offsets_ok("nobsm_off", noff, Nz, "nobsm", ntxt.n) || !offsets_ok("tok_off", t.tok_off, NK, "tok", t.tok.n) ||
        !offsets_ok("piece_off", t.piece_off, QV_VOCAB, "piece_codes", pcodes.n) || !offsets_ok("vtri_off", t.vtri_off, Nz, "vtri", t.vtri.n))
        return QV_ERR_IO;
    // the counts uploaded (and indexed) are the file's own, not the sections' sizes
    t.surah.n = t.ayah.n = t.nw[0].n = t.nw[1].n = t.nw[2].n = Nz;
    t.surah_start.n = (size_t)NS + 1; t.surah_len.n = (size_t)NS;
    t.tri_keys.n = t.tri_idf.n = (size_t)NT;
    t.vtri_off.n = Nz + 1; t.vtri.n = t.vtri_off[Nz];
    t.tok_off.n = NK + 1; t.tok.n = t.tok_off[NK];
    t.piece_off.n = (size_t)QV_VOCAB + 1;
    const struct { const char *name; const QvView<uint32_t> &off; } texts[3] = {{"clean", coff}, {"alt", aoff}, {"nobsm", noff}};
    for (const auto &x : texts)
        for (size_t v = 0; v < Nz; ++v)
            if (x.off[v + 1] - x.off[v] > QV_MAX_TEXT)
                return fail(std::string("tables: ") + x.name + " text of verse " + std::to_string(v) + " has " + std::to_string(x.off[v + 1] - x.off[v]) +
                            " codes, the kernels take " + std::to_string(QV_MAX_TEXT));
    if (qv_largest(t.tok.p, t.tok.n) >= QV_VOCAB) return fail("tables: tok holds token id " + std::to_string(qv_largest(t.tok.p, t.tok.n)) + " (vocabulary " + std::to_string(QV_VOCAB) + ")");
    if (t.vtri.n && qv_largest(t.vtri.p, t.vtri.n) >= NT) return fail("tables: vtri holds a trigram id out of range");
    if (qv_largest(t.tri_keys.p, t.tri_keys.n) >= (1u << 18)) return fail("tables: tri_keys holds a trigram key out of range");
    for (int s = 0; s <= NS; ++s)
        if (t.surah_start[s] < 0 || t.surah_start[s] > N || (s && t.surah_start[s] < t.surah_start[s - 1]))
            return fail("tables: surah_start is not a non-decreasing sequence within the verses");
    for (int s = 0; s < NS; ++s)
        if (t.surah_len[s] < 0 || t.surah_len[s] > N - t.surah_start[s]) return fail("tables: surah_len reaches past the verses");

    t.h_surah.assign(t.surah.p, t.surah.p + N);
    t.h_ayah.assign(t.ayah.p, t.ayah.p + N);
    // padded clean array: verse texts separated by one space
    std::vector<uint8_t> &cpad = t.clean;
    std::vector<uint32_t> &cpo = t.clean_off, &apo = t.alt_off;
    std::vector<uint16_t> &clen = t.clean_len, &alen = t.alt_len, &nlen = t.nobsm_len;
    std::vector<int32_t> &nrank = t.nobsm_rank;
    cpo.resize(N); apo.resize(N);
    clen.resize(N); alen.resize(N); nlen.resize(N);
    nrank.assign(N, -1);
    int n_nobsm = 0;
    for (int v = 0; v < N; ++v) {
        cpo[v] = (uint32_t)cpad.size();
        clen[v] = (uint16_t)(coff[v + 1] - coff[v]);
        cpad.insert(cpad.end(), ctxt.p + coff[v], ctxt.p + coff[v + 1]);
        cpad.push_back(0);
        apo[v] = aoff[v];
        alen[v] = (uint16_t)(aoff[v + 1] - aoff[v]);
        nlen[v] = (uint16_t)(noff[v + 1] - noff[v]);
        if (nlen[v]) {
            nrank[v] = n_nobsm++;
            // the no-bismillah text must be a suffix of the clean text (it is clean[len(BSM):].strip())
            if (nlen[v] > clen[v] || memcmp(ntxt.p + noff[v], ctxt.p + coff[v + 1] - nlen[v], nlen[v]) != 0)
                return fail("tables: no_bsm text is not a suffix of text_clean");
        }
    }
    {
        std::vector<uint8_t> &c8 = t.clean8;
        std::vector<uint32_t> &o8 = t.clean8_off;
        o8.resize(N + 1);
        for (int v = 0; v < N; ++v) {
            o8[v] = (uint32_t)c8.size();
            c8.push_back(0);
            c8.insert(c8.end(), ctxt.p + coff[v], ctxt.p + coff[v + 1]);
            while (c8.size() & 7) c8.push_back(0xFF);
        }
        o8[N] = (uint32_t)c8.size();
        c8.resize(c8.size() + 64, 0xFF);
    }
    cpad.resize(cpad.size() + 64, 0);
    t.alt.assign(atxt.p, atxt.p + aoff[N]);
    t.alt.resize(t.alt.size() + 64, 0);  // texts are read 8 bytes at a time
    {   // word ends of the clean texts (the verse tracker's prefix scores)
        std::vector<uint32_t> &wo = t.wend_off;
        std::vector<uint16_t> &we = t.wend;
        wo.assign(N + 1, 0);
        const QvView<uint16_t> &cnw = t.nw[0];
        for (int v = 0; v < N; ++v) {
            wo[v] = (uint32_t)we.size();
            for (int i = 0; i < clen[v]; ++i)
                if (ctxt[coff[v] + i] == 0) we.push_back((uint16_t)i);
            we.push_back(clen[v]);
            if ((int)(we.size() - wo[v]) != cnw[v]) return fail("tables: clean_nw disagrees with the text");
        }
        wo[N] = (uint32_t)we.size();
        std::vector<int32_t> &order = t.len_order;
        order.resize(N);
        for (int v = 0; v < N; ++v) order[v] = v;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return clen[a] > clen[b]; });
    }
    // per-text match masks
    t.n_text = 2 * N + n_nobsm;
    std::vector<uint32_t> &pmo = t.pmv_off;
    std::vector<uint64_t> &pmv = t.pmv;
    pmo.resize(t.n_text);
    auto add_text = [&](int tid, const uint8_t *s, int len) {
        int stride = qv_tmpl_w((len + 63) / 64);
        pmo[tid] = (uint32_t)pmv.size();
        pmv.resize(pmv.size() + (size_t)QV_NSYM * stride, 0ull);
        uint64_t *base = pmv.data() + pmo[tid];
        for (int i = 0; i < len; ++i)
            if (s[i] < QV_NSYM) base[(size_t)s[i] * stride + (i >> 6)] |= 1ull << (i & 63);
    };
    for (int v = 0; v < N; ++v) add_text(v, ctxt.p + coff[v], clen[v]);
    for (int v = 0; v < N; ++v) add_text(N + v, atxt.p + aoff[v], alen[v]);
    for (int v = 0; v < N; ++v)
        if (nlen[v]) add_text(2 * N + nrank[v], ntxt.p + noff[v], nlen[v]);
    pmv.resize(pmv.size() + 16, 0ull);
    {   // inverted trigram index, split in four verse-range slices (one per wave of k_trigram)
        const QvView<uint32_t> &vto = t.vtri_off;
        const QvView<uint16_t> &vt = t.vtri;
        std::vector<uint32_t> start(NT + 1, 0);
        for (uint32_t p = 0; p < vto[N]; ++p) ++start[vt[p] + 1];
        for (int i = 0; i < NT; ++i) start[i + 1] += start[i];
        std::vector<uint16_t> &post = t.tri_post;
        post.assign(vto[N] + 64, 0);
        std::vector<uint32_t> fill(start.begin(), start.end() - 1), &slice = t.tri_slice;
        slice.resize((size_t)NT * 5);
        for (int i = 0; i < NT; ++i) slice[(size_t)i * 5] = start[i];
        int w = 0;
        for (int v = 0; v < N; ++v) {
            while (w < 3 && v >= (int)((long long)(w + 1) * N / 4)) {   // verse v opens slice w + 1
                ++w;
                for (int i = 0; i < NT; ++i) slice[(size_t)i * 5 + w] = fill[i];
            }
            for (uint32_t p = vto[v]; p < vto[v + 1]; ++p) post[fill[vt[p]]++] = (uint16_t)v;
        }
        for (++w; w <= 4; ++w)
            for (int i = 0; i < NT; ++i) slice[(size_t)i * 5 + w] = fill[i];
        std::vector<uint16_t> &map = t.tri_map;
        map.assign((size_t)1 << 18, 0xFFFF);
        for (int i = 0; i < NT; ++i) map[t.tri_keys[i]] = (uint16_t)i;
    }
    {   // prefix flags of the token table (see QvTables::tok_pfx)
        const QvView<uint32_t> &to = t.tok_off;
        const uint16_t *tk = t.tok.p;
        std::vector<uint8_t> &pfx = t.tok_pfx;
        pfx.assign(N, 0);
        for (int v = 0; v < N; ++v)
            for (int k = 1; k < QV_MAX_SPAN; ++k) {
                const uint32_t a0 = to[(size_t)v * QV_MAX_SPAN + k - 1], a1 = to[(size_t)v * QV_MAX_SPAN + k], b1 = to[(size_t)v * QV_MAX_SPAN + k + 1];
                const uint32_t la = a1 - a0, lb = b1 - a1;
                if (la > 0 && lb >= la && memcmp(tk + a0, tk + a1, sizeof(uint16_t) * la) == 0) pfx[v] |= (uint8_t)(1u << (k - 1));
            }
    }
    // the kernels read a piece's codes up to 16 bytes past its end: the padding is part of the array
    t.piece_codes.assign(pcodes.p, pcodes.p + t.piece_off[QV_VOCAB]);
    t.piece_codes.resize(t.piece_codes.size() + 16, 0);
    return QV_OK;
}

// The tables file at `path`, read whole and built: QV_OK with `out` filled (it owns the bytes its views point into), else
// the code and `err`.  A file that is empty or cannot be read to its end is refused by the bad-magic rule above.
inline int qv_read_host_tables(const char *path, HostTables &out, std::string &err) {
    std::vector<uint8_t> file;
    {
        std::ifstream f;
        if (path) f.open(path, std::ios::binary | std::ios::ate);
        if (!path || !f) { err = std::string("cannot open tables file: ") + (path ? path : "(null)"); return QV_ERR_IO; }
        const std::streamsize sz = f.tellg();
        f.seekg(0);
        file.resize(sz > 0 ? (size_t)sz : 0);
        if (!f.read((char *)file.data(), (std::streamsize)file.size())) file.clear();
    }
    const int rc = qv_build_host_tables(file.data(), file.size(), out, err);
    if (rc == QV_OK) out.file = std::move(file);   // (a moved vector keeps its storage: the views stay valid)
    return rc;
}
