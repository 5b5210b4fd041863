// tests/emu/col_decode_check.cpp — TEST ONLY: metagraph_amd/csrc/col_decode.hpp (the kernel bodies behind
// mgx_annotation_load_columns_device) run on the host, one call per item in the order of the launches of mgx_colload.hip, over the
// plan and the batch layout of col_plan.hpp.  Built with -fsanitize=address,undefined by tests/test_col_decode_model.py; every
// array has exactly the size the driver gives its device buffer, so that an access the kernels would make outside a buffer stops
// the program.
// usage: col_decode_check OUT.bin IN.column.annodbg [IN ...] [-- OUT.bin IN ...]; one line per group:
//   "ok <n_rows> <n_labels>" (OUT.bin: n_rows, n_labels as u64, per label its length as u64 and its bytes, col_begin, rows),
//   "invalid <message>", "unsupported <message>" — the host reader's answer wherever the plan or a check asks for it — or
//   "internal <message>" where the device path refuses what the host reader accepts.
#include "wave.hpp"
#include "../../metagraph_amd/csrc/col_decode.hpp"
#include "../../metagraph_amd/csrc/col_plan.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace mgx;
using namespace mgx::files;

typedef std::vector<uint64_t> Words;

static void scan(Words &d) {
    uint64_t s = 0;
    for (uint64_t &x : d) { const uint64_t c = x; x = s; s += c; }
}

// mgx_column_file_read: the files side by side
static ColumnFile host_read(const std::vector<std::string> &paths) {
    ColumnFile m;
    std::set<std::string> seen;
    for (size_t i = 0; i < paths.size(); ++i) {
        const ColumnFile f = read_columns(paths[i]);
        if (i && f.n_rows != m.n_rows) throw ParseError("annotates " + std::to_string(f.n_rows) + " rows, the files before it " + std::to_string(m.n_rows));
        m.n_rows = f.n_rows;
        for (size_t j = 0; j < f.labels.size(); ++j) {
            if (!seen.insert(f.labels[j]).second) throw Unsupported("label '" + f.labels[j] + "' occurs in two files");
            m.labels.push_back(f.labels[j]);
            m.rows.insert(m.rows.end(), f.rows.begin() + (std::ptrdiff_t)f.col_begin[j], f.rows.begin() + (std::ptrdiff_t)f.col_begin[j + 1]);
            m.col_begin.push_back(m.rows.size());
        }
    }
    return m;
}

static void dump(const std::string &out_path, const ColumnFile &f) {
    FILE *o = fopen(out_path.c_str(), "wb");
    if (!o) { printf("invalid cannot write %s\n", out_path.c_str()); return; }
    const uint64_t hdr[2] = { f.n_rows, f.labels.size() };
    fwrite(hdr, 8, 2, o);
    for (const std::string &l : f.labels) { const uint64_t n = l.size(); fwrite(&n, 8, 1, o); fwrite(l.data(), 1, l.size(), o); }
    fwrite(f.col_begin.data(), 8, f.col_begin.size(), o);
    if (!f.rows.empty()) fwrite(f.rows.data(), 8, f.rows.size(), o);
    fclose(o);
    printf("ok %llu %llu\n", (unsigned long long)f.n_rows, (unsigned long long)f.labels.size());
}

// the host reader's verdict where the device path asks for it
static void host_answer(const std::vector<std::string> &paths, const std::string &why) {
    try {
        host_read(paths);
        printf("internal the device decode refuses (%s) a file that the host reader accepts\n", why.c_str());
    } catch (const Unsupported &e) {
        printf("unsupported %s\n", e.what());
    } catch (const ParseError &e) {
        printf("invalid %s\n", e.what());
    }
}

static void one(const std::string &out_path, const std::vector<std::string> &paths) {
    std::vector<std::vector<uint8_t>> images(paths.size());
    std::vector<ColumnsPlan> plans(paths.size());
    ColBatch b;
    try {
        for (size_t i = 0; i < paths.size(); ++i) {
            images[i] = read_whole_file(paths[i]);              // at its exact size on the heap: the plan's spans are checked against it
            plans[i] = plan_columns(images[i].data(), images[i].size());
        }
        check_merge(plans);
        uint64_t n_labels = 0;
        for (const ColumnsPlan &p : plans) n_labels += p.labels.size();
        if (!plans[0].n_rows || !n_labels || n_labels >= (1u << 24)) { dump(out_path, host_read(paths)); return; }
        b.build(plans);
    } catch (const std::runtime_error &e) {
        host_answer(paths, e.what());
        return;
    }
    images.clear();
    const uint32_t n_labels = (uint32_t)b.lab.size(), n_sd = (uint32_t)b.sd.size();
    const uint64_t HW = b.high_words(), BW = b.bm_words(), RB = b.rrr_blocks();
    uint64_t err = DD_NO_ERROR;
    Words arena(b.arena_words, 0);
    if (b.upload_words) memcpy(arena.data(), b.stage.data(), b.upload_words * 8);
    uint64_t *A = arena.data();
    // (copies at their exact sizes: a std::vector's data() of an empty table is not dereferenced by a correct body)
    const std::vector<CdRrr> rd(b.rrr);
    const std::vector<CdSd> sd(b.sd);
    const std::vector<CdBm> bm(b.bm);
    const std::vector<CdLabel> lab(b.lab);
    const Words hprefix(b.hprefix);
    Words hrank(HW + 1), bscan(BW + 1), counts(n_labels);
    if (RB) {
        const auto &C = binomial63().c;
        std::vector<uint8_t> wtab(64);
        Words binom(DD_BINOM_ENTRIES), off(RB + 1), blocks(RB);
        for (unsigned k = 0; k < 64; ++k) wtab[k] = (k == 0 || k == 63) ? 0 : (uint8_t)(64 - __builtin_clzll(C[63][k]));
        for (unsigned n = 0; n < 63; ++n) for (unsigned j = 0; j < 32; ++j) binom[n * 32 + j] = C[n][j];
        for (uint64_t gb = 0; gb <= RB; ++gb) off[gb] = cd_rrr_width(A, rd.data(), wtab.data(), gb, b.n_blocks, rd.size());
        scan(off);
        for (uint64_t gb = 0; gb < RB; ++gb) blocks[gb] = cd_rrr_block(A, rd.data(), off.data(), wtab.data(), binom.data(), gb, b.n_blocks, &err);
        for (uint64_t g = 0; g < rd.size() * b.W; ++g) cd_rrr_pack(A, rd.data(), blocks.data(), g, b.W, b.n_blocks, b.n_rows);
    }
    if (n_sd) {
        for (uint64_t gw = 0; gw <= HW; ++gw) hrank[gw] = cd_high_popcount(A, sd.data(), hprefix.data(), n_sd, gw);
        scan(hrank);
        if (b.kinds[CD_KIND_SD_INVERTED])
            for (uint64_t gw = 0; gw < HW; ++gw) cd_sd_word(A, sd.data(), hprefix.data(), n_sd, hrank.data(), gw, b.n_rows, 0, nullptr, nullptr, &err);
    }
    if (BW) {
        for (uint64_t g = 0; g <= BW; ++g) bscan[g] = cd_bm_popcount(A, bm.data(), g, bm.size(), b.W, b.n_rows, &err);
        scan(bscan);
    }
    for (uint32_t j = 0; j < n_labels; ++j)
        counts[j] = cd_count(lab.data(), sd.data(), bm.data(), hprefix.data(), hrank.data(), bscan.data(), j, b.W, b.n_rows, &err);
    ColumnFile f;
    if (err == DD_NO_ERROR && !b.col_begin_from(counts, f.col_begin)) { host_answer(paths, "more than 2^33 expanded rows"); return; }
    if (err == DD_NO_ERROR) {
        f.rows.resize(f.col_begin.back());
        const Words cb(f.col_begin);
        if (b.kinds[CD_KIND_SD])
            for (uint64_t gw = 0; gw < HW; ++gw) cd_sd_word(A, sd.data(), hprefix.data(), n_sd, hrank.data(), gw, b.n_rows, 1, cb.data(), f.rows.data(), &err);
        for (uint64_t g = 0; g < BW; ++g) cd_bm_extract(A, bm.data(), bscan.data(), g, b.W, b.n_rows, cb.data(), f.rows.data(), &err);
    }
    if (err != DD_NO_ERROR) {
        host_answer(paths, "column " + std::to_string(err >> 40) + ", check " + std::to_string((err >> 32) & 0xFF) + " at " + std::to_string(err & 0xFFFFFFFFu));
        return;
    }
    f.n_rows = b.n_rows;
    f.labels = b.labels;
    dump(out_path, f);
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s OUT.bin IN.column.annodbg [IN ...] [-- OUT.bin IN ...]\n", argv[0]); return 2; }
    for (int a = 1; a < argc;) {
        const std::string out = argv[a++];
        std::vector<std::string> in;
        for (; a < argc && std::string(argv[a]) != "--"; ++a) in.push_back(argv[a]);
        ++a;
        if (in.empty()) { fprintf(stderr, "no input for %s\n", out.c_str()); return 2; }
        one(out, in);
    }
    return 0;
}
