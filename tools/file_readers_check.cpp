// dev / test: the two file readers behind qv_create (csrc/qv_tables_host.h, csrc/qv_weights_host.h) -- host only, no GPU.
//
//     c++ -std=c++17 -fsanitize=address,undefined tools/file_readers_check.cpp -o file_readers_check
//     ./file_readers_check tables offline-tarteel_amd/data/qverse_tables.bin [--dump DIR]
//     ./file_readers_check weights weights.bin
//
// Exit status 0 and the counts on stdout when the file is accepted, 3 and the reader's message when it is refused, 2 for a
// bad command line.  --dump writes every derived array as a raw file named after its QvTables member.
// tests/test_file_readers_host.py builds and runs it.
#include "../offline-tarteel_amd/csrc/qv_tables_host.h"
#include "../offline-tarteel_amd/csrc/qv_weights_host.h"

#include <stdio.h>

#include <fstream>
#include <string>
#include <vector>

namespace {

template <typename V>
bool dump(const std::string &dir, const char *name, const V &v) {
    std::ofstream f(dir + "/" + name, std::ios::binary);
    f.write((const char *)v.data(), (std::streamsize)(v.size() * sizeof(*v.data())));
    return (bool)f;
}

int refused(const std::string &err) {
    printf("refused: %s\n", err.c_str());
    return 3;
}

int check_tables(const char *path, const char *dump_dir) {
    HostTables h;
    std::string err;
    if (qv_read_host_tables(path, h, err) != QV_OK) return refused(err);
    printf("tables ok: n_verses %d n_surah %d n_tri %d n_text %d\n", h.n_verses, h.n_surah, h.n_tri, h.n_text);
    if (!dump_dir) return 0;
    const std::string d = dump_dir;
#define DUMP(member) if (!dump(d, #member, h.member)) { fprintf(stderr, "cannot write %s/%s\n", dump_dir, #member); return 2; }
    DUMP(clean) DUMP(clean_off) DUMP(clean_len) DUMP(nobsm_len) DUMP(clean8) DUMP(clean8_off) DUMP(alt) DUMP(alt_off) DUMP(alt_len)
    DUMP(nobsm_rank) DUMP(wend_off) DUMP(wend) DUMP(len_order) DUMP(pmv) DUMP(pmv_off) DUMP(tri_post) DUMP(tri_map) DUMP(tri_slice)
    DUMP(tok_pfx) DUMP(piece_codes)
#undef DUMP
    return 0;
}

int check_weights(const char *path) {
    HostWeights hw;
    std::string err;
    if (load_weight_file(path, hw, err) != QV_OK) return refused(err);
    printf("weights ok: %zu tensors\n", hw.t.size());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc >= 3 ? argv[1] : "";
    if (mode == "tables" && (argc == 3 || (argc == 5 && std::string(argv[3]) == "--dump"))) return check_tables(argv[2], argc == 5 ? argv[4] : nullptr);
    if (mode == "weights" && argc == 3) return check_weights(argv[2]);
    fprintf(stderr, "usage: file_readers_check tables <path> [--dump <dir>] | weights <path>\n");
    return 2;
}
