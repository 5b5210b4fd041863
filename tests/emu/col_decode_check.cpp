// tests/emu/col_decode_check.cpp — TEST ONLY: metagraph_amd/csrc/bv_decode.hpp and col_decode.hpp (the kernel bodies behind
// mgx_annotation_load_columns_device) run on the host in the order of the launches of mgx_colload.hip (bv_stage.hpp), over the
// plan and the batch layout of col_plan.hpp.  Built with -fsanitize=address,undefined by tests/test_col_decode_model.py; every
// array has exactly the size the driver gives its device buffer, so that an access the kernels would make outside a buffer stops
// the program.
// usage: col_decode_check OUT.bin IN.column.annodbg [IN ...] [-- OUT.bin IN ...]; one line per group:
//   "ok <n_rows> <n_labels>" (OUT.bin: n_rows, n_labels as u64, per label its length as u64 and its bytes, col_begin, rows),
//   "invalid <message>", "unsupported <message>" — the host reader's answer wherever the plan or a check asks for it — or
//   "internal <message>" where the device path refuses what the host reader accepts.
#include "wave.hpp"
#include "bv_stage.hpp"

#include <cstdio>
#include <string>

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
    uint64_t err = DD_NO_ERROR;
    Words arena(b.arena_words, 0);
    if (b.upload_words) memcpy(arena.data(), b.stage.data(), b.upload_words * 8);
    uint64_t *A = arena.data();
    BvHost d(b.v);
    bv_stage(A, b.v, d, &err);
    const Words counts = col_counts(A, b, d, &err);
    ColumnFile f;
    if (err == DD_NO_ERROR && !b.col_begin_from(counts, f.col_begin)) { host_answer(paths, "more than 2^33 expanded rows"); return; }
    if (err == DD_NO_ERROR) {
        f.rows.resize(f.col_begin.back());
        col_rows(A, b, d, Words(f.col_begin), f.rows.data(), &err);
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
