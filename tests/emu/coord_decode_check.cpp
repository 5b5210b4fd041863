// tests/emu/coord_decode_check.cpp — TEST ONLY: metagraph_amd/csrc/coord_decode.hpp (the kernel bodies behind
// mgx_annotation_load_coord_columns_device and mgx_annotation_set_coordinates_device) behind the stages of bv_stage.hpp, run on
// the host, one call per item in the order of the launches of mgx_colload.hip and mgx_annot.hip, over the plans and batch
// layouts of col_plan.hpp / coord_plan.hpp.  Every array has exactly the size the driver gives its device buffer; built by
// tests/test_coord_decode_model.py (with -fsanitize=address,undefined an access outside a buffer stops the program).
// usage: coord_decode_check OUT.bin IN [IN ...] [-- OUT.bin IN ...]; IN: `.column.annodbg` files with their `.coords` side files
// next to them, or one `.column_coord.annodbg`.  One line per group:
//   "ok <n_rows> <n_labels>" (OUT.bin: n_rows, n_labels, n_entries, n_coords as u64, per label its length as u64 and its bytes,
//   col_begin, rows, coord_begin, coords), "invalid <message>", "unsupported <message>" — the host reader's answer wherever the
//   plan or a check asks for it — or "internal <message>" where the device path refuses what the host reader accepts, or where
//   the transposition's tables differ from the ones mgx_annotation_set_coordinates builds.
#include "wave.hpp"
#include "bv_stage.hpp"
#include "../../metagraph_amd/csrc/column_file.hpp"
#include "../../metagraph_amd/csrc/coord_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <string>

// mgx_column_coord_file_read
static ColumnFile host_read(const std::vector<std::string> &paths) {
    for (const std::string &p : paths) if (is_column_coord_path(p) && paths.size() > 1) throw ParseError("a .column_coord.annodbg file is loaded alone");
    if (is_column_coord_path(paths[0])) {
        const std::vector<uint8_t> buf = read_whole_file(paths[0]);
        return parse_column_coord(buf.data(), buf.size());
    }
    ColumnFile m;
    m.coord_begin.push_back(0);
    m.has_coords = true;
    std::set<std::string> seen;
    for (size_t i = 0; i < paths.size(); ++i) {
        ColumnFile f = read_columns(paths[i]);
        if (i && f.n_rows != m.n_rows) throw ParseError("annotates " + std::to_string(f.n_rows) + " rows, the files before it " + std::to_string(m.n_rows));
        for (const std::string &l : f.labels) if (!seen.insert(l).second) throw Unsupported("label '" + l + "' occurs in two files");
        const std::vector<uint8_t> sb = read_whole_file(coord_side_path(paths[i]));
        Cursor c(sb.data(), sb.size());
        read_tuples(c, f, 0, f.labels.size());
        m.n_rows = f.n_rows;
        const uint64_t row0 = m.rows.size(), coord0 = m.coords.size();
        m.labels.insert(m.labels.end(), f.labels.begin(), f.labels.end());
        m.rows.insert(m.rows.end(), f.rows.begin(), f.rows.end());
        for (size_t j = 1; j < f.col_begin.size(); ++j) m.col_begin.push_back(row0 + f.col_begin[j]);
        for (size_t e = 1; e < f.coord_begin.size(); ++e) m.coord_begin.push_back(coord0 + f.coord_begin[e]);
        m.coords.insert(m.coords.end(), f.coords.begin(), f.coords.end());
    }
    return m;
}

static void dump(const std::string &out_path, const ColumnFile &f) {
    FILE *o = fopen(out_path.c_str(), "wb");
    if (!o) { printf("invalid cannot write %s\n", out_path.c_str()); return; }
    const uint64_t hdr[4] = { f.n_rows, f.labels.size(), f.rows.size(), f.coords.size() };
    fwrite(hdr, 8, 4, o);
    for (const std::string &l : f.labels) { const uint64_t n = l.size(); fwrite(&n, 8, 1, o); fwrite(l.data(), 1, l.size(), o); }
    fwrite(f.col_begin.data(), 8, f.col_begin.size(), o);
    if (!f.rows.empty()) fwrite(f.rows.data(), 8, f.rows.size(), o);
    fwrite(f.coord_begin.data(), 8, f.coord_begin.size(), o);
    if (!f.coords.empty()) fwrite(f.coords.data(), 8, f.coords.size(), o);
    fclose(o);
    printf("ok %llu %llu\n", (unsigned long long)f.n_rows, (unsigned long long)f.labels.size());
}

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

// mgx_annotation_set_coordinates_device in launch order; false: its error record was set (*err_out).  Compared with the tables
// mgx_annotation_set_coordinates builds (the sort of (row, label, entry) records).
static bool transpose(const ColumnFile &f, uint64_t *err_out, std::string *diff) {
    const uint64_t n_entries = f.rows.size(), n_coords = f.coords.size(), n_rows = f.n_rows;
    const uint32_t n_labels = (uint32_t)f.labels.size();
    uint64_t err = CT_NO_ERROR;
    const Words cb(f.col_begin), rows(f.rows), cob(f.coord_begin);
    const std::vector<int64_t> co(f.coords);
    for (uint64_t i = 0; i < std::max(n_entries, n_coords); ++i) ct_check(rows.data(), n_entries, n_rows, cob.data(), co.data(), n_coords, i, &err);
    Words keys(n_entries), perm(n_entries);
    for (uint64_t x = 0; x < n_entries; ++x) ct_key(cb.data(), n_labels, rows.data(), n_rows, x, keys.data(), perm.data());
    std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });      // (the stable radix sort by key)
    Words keys_s(n_entries);
    for (uint64_t e = 0; e < n_entries; ++e) keys_s[e] = keys[perm[e]];
    *err_out = err;
    if (err != CT_NO_ERROR) return false;
    Words row_entry(n_rows + 1, 0), coord_off(n_entries + 1);
    for (uint64_t e = 0; e < n_entries; ++e) ct_row_count(keys_s.data(), n_entries, n_rows, e, row_entry.data());
    for (uint64_t e = 0; e <= n_entries; ++e) coord_off[e] = ct_tuple_len(perm.data(), cob.data(), n_entries, n_coords, e);
    scan(row_entry);
    scan(coord_off);
    const uint64_t total = coord_off[n_entries];
    std::vector<int64_t> flat(total);
    for (uint64_t o = 0; o < total; ++o) ct_copy(coord_off.data(), perm.data(), cob.data(), co.data(), n_entries, n_coords, o, flat.data());
    // mgx_annotation_set_coordinates
    std::vector<std::pair<std::pair<uint64_t, uint32_t>, uint64_t>> order;
    for (uint32_t j = 0; j < n_labels; ++j) for (uint64_t x = cb[j]; x < cb[j + 1]; ++x) order.push_back({ { rows[x], j }, x });
    std::sort(order.begin(), order.end());
    Words want_entry(n_rows + 1, 0), want_off(n_entries + 1, 0);
    std::vector<int64_t> want_flat;
    for (uint64_t e = 0; e < n_entries; ++e) {
        ++want_entry[order[e].first.first + 1];
        for (uint64_t c = cob[order[e].second]; c < cob[order[e].second + 1]; ++c) want_flat.push_back(co[c]);
        want_off[e + 1] = want_flat.size();
    }
    for (uint64_t r = 0; r < n_rows; ++r) want_entry[r + 1] += want_entry[r];
    if (row_entry != want_entry) *diff = "row_entry";
    else if (coord_off != want_off) *diff = "coord_off";
    else if (flat != want_flat) *diff = "coords";
    return true;
}

static void one(const std::string &out_path, const std::vector<std::string> &paths) {
    const size_t n_paths = paths.size();
    std::vector<std::vector<uint8_t>> images(n_paths), sides(n_paths);
    std::vector<ColumnsPlan> plans(n_paths);
    std::vector<std::vector<TuplePlan>> tuples(n_paths);
    ColBatch b;
    CoordBatch cq;
    try {
        for (size_t i = 0; i < n_paths; ++i) {
            images[i] = read_whole_file(paths[i]);              // at its exact size on the heap: the plan's spans are checked against it
            if (is_column_coord_path(paths[i])) {
                if (n_paths > 1) throw NeedsHost("a .column_coord.annodbg file next to others");
                plans[i] = plan_column_coord(images[i].data(), images[i].size(), tuples[i]);
                continue;
            }
            plans[i] = plan_columns(images[i].data(), images[i].size());
            sides[i] = read_whole_file(coord_side_path(paths[i]));
            Cursor c(sides[i].data(), sides[i].size());
            tuples[i] = plan_tuples(c, sides[i].data(), plans[i].labels.size(), plans[i].n_rows);
        }
        check_merge(plans);
        uint64_t n_labels = 0;
        for (const ColumnsPlan &p : plans) n_labels += p.labels.size();
        if (!plans[0].n_rows || !n_labels || n_labels >= (1u << 24)) { dump(out_path, host_read(paths)); return; }
        std::vector<const TuplePlan *> tp;
        for (const std::vector<TuplePlan> &v : tuples) for (const TuplePlan &t : v) tp.push_back(&t);
        cq.layout(tp);
        b.build(plans, cq.upload_words);
        cq.place(tp, b.extra_begin, b.arena_words, b.stage.data());
    } catch (const std::runtime_error &e) {
        host_answer(paths, e.what());
        return;
    }
    images.clear();
    sides.clear();
    uint64_t err = DD_NO_ERROR;
    Words arena(b.arena_words + cq.v.tail_words, 0);
    if (b.upload_words) memcpy(arena.data(), b.stage.data(), b.upload_words * 8);
    uint64_t *A = arena.data();
    BvHost d(b.v);
    bv_stage(A, b.v, d, &err);
    const Words counts = col_counts(A, b, d, &err);
    ColumnFile f;
    if (err == DD_NO_ERROR && !b.col_begin_from(counts, f.col_begin)) { host_answer(paths, "more than 2^33 expanded rows"); return; }
    if (err == DD_NO_ERROR && !cq.lengths_fit(f.col_begin)) { host_answer(paths, "delimiters: length"); return; }
    if (err == DD_NO_ERROR) {
        f.rows.resize(f.col_begin.back());
        const Words cb(f.col_begin);
        col_rows(A, b, d, cb, f.rows.data(), &err);
        // ---- the tuple sections (decode_coords) ----
        const uint32_t n_cols = (uint32_t)cq.col.size();
        const uint64_t NV = cq.n_values();
        const std::vector<CqCol> qcol(cq.col);
        const Words qv(cq.vprefix);
        BvHost q(cq.v);
        bv_stage(A, cq.v, q, &err);
        for (uint32_t j = 0; j < n_cols; ++j)
            cq_check(A, q.map.data(), qcol.data(), q.sd.data(), q.hprefix.data(), q.hrank.data(), q.bmprefix.data(), q.bscan.data(), cb.data(), j, &err);
        f.coord_begin.assign(f.rows.size() + 1, ~0ull);
        f.coords.assign(NV, -1);
        for (uint64_t g = 0; g < q.BW; ++g)
            cq_rank(A, q.map.data(), q.bmprefix.data(), n_cols, q.bscan.data(), cb.data(), qv.data(), g, f.coord_begin.data(), &err);
        for (uint64_t o = 0; o < NV; ++o) cq_unpack(A, qcol.data(), qv.data(), n_cols, o, f.coords.data(), &err);
    }
    if (err != DD_NO_ERROR) {
        host_answer(paths, "column " + std::to_string(err >> 40) + ", check " + std::to_string((err >> 32) & 0xFF) + " at " + std::to_string(err & 0xFFFFFFFFu));
        return;
    }
    f.n_rows = b.n_rows;
    f.labels = b.labels;
    f.has_coords = true;
    uint64_t terr = CT_NO_ERROR;
    std::string diff;
    if (!transpose(f, &terr, &diff)) { host_answer(paths, terr >> 62 ? "a tuple is not ascending" : "a row outside the matrix"); return; }
    if (!diff.empty()) { printf("internal the transposition's %s differ from mgx_annotation_set_coordinates'\n", diff.c_str()); return; }
    dump(out_path, f);
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s OUT.bin IN [IN ...] [-- OUT.bin IN ...]\n", argv[0]); return 2; }
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
