// mgx_align — minimal `metagraph align`-shaped driver over HipDBGAligner (host side only: batching and
// TSV printing as in cli/align.cpp:403-480).  Graph input: a `.dbg` file written by the reference (mgx_boss_file_read:
// SMALL / STAT / FAST state, DNA; the graph's mode is the file's) or a flat BOSS dump (k, n_edges, F[5], W[], last[]).  Usage:
//   mgx_align GRAPH.{dbg,boss} READS.{fa,fq} [--align-only-forwards] [--align-min-exact-match X] [--align-min-seed-length N]
//             [-p THREADS] [--query-batch-size BASES] [--canonical | --primary (the dump is a CANONICAL- / PRIMARY-mode graph)]
//             [--time]        wall time of the align loop on stderr
//             [--map]         map_sequences_in_file (cli/align.cpp:71-179) instead of aligning: "{k-mer}: {node}" per k-mer, or with
//                             --count-kmers "{name}\t{discovered}/{k-mers}/{distinct}", --query-presence "0" / "1",
//                             --query-presence --filter-present the present records as FASTA; --discovery-fraction X (0.7);
//                             --align-length N (windows of N < k characters; 0 = k, above k: a warning and k);
//                             --fwd-and-reverse (every record followed by its reverse complement under the same name).
//                             Output in input order; no annotation is loaded in this mode
//             [--map-on-device]  with --map: every batch is mapped with its node array left in device memory and its text is written
//                             by kernels (mgx_format_map_batch) and printed with one write per batch; same bytes in every form.
//                             With --parse-on-device in addition (not --format-on-device): the file is read in chunks and parsed by
//                             kernels as for alignment (same grammar, same two exceptions), the reads are mapped from the parser's
//                             device arrays — file bytes in, text bytes out; -p 1 and --devices 1 only, not with --fwd-and-reverse
//                             (whose records are made on the host).  --parse-chunk-bytes and --time work as for alignment.
//                             A third exception on this path: a name that holds a NUL byte is printed whole (the host path
//                             and mgx_format_map cut a name at its first NUL)
//             [--format-on-device]  the TSV text of every batch is written by kernels (mgx_format_tsv_batch) and printed with one write
//                             per batch, instead of one host-built string per query; same bytes.  Not with --map or --rccl-gather
//             [--json]        the lines of `metagraph align --json` (cli/align.cpp:287-305) instead of TSV: one JSON object per
//                             alignment, a {"name":..,"sequence":""} object for a query without one; input order with -p 1.  Without
//                             --format-on-device: mgx_fetch_results and mgx_format_json per query.  With --format-on-device: written by
//                             kernels (mgx_format_json_batch), a batch in slices, one write per slice; with --parse-on-device in
//                             addition as for TSV.  Same bytes in every form.  Labels are not printed (JSON carries none).  Not with
//                             --map or --rccl-gather, nor with post_chain_alignments (the reference has no JSON for chains)
//             [--json-slice-bytes N]  with --json --format-on-device: JSON text is ~100 bytes per query character (one mapping object per
//                             path node), so a batch is formatted in slices: consecutive queries are added to a slice while its
//                             ESTIMATED text — (128 bytes per character + twice the header + 512) x num_alternative_paths per
//                             query — stays within N (default 268435456; a slice always takes at least one query).  The estimate is
//                             an upper bound for reads without long insertions or many escaped bytes; the output does not depend on N
//             [--parse-on-device]  with --format-on-device, -p 1 and --devices 1: the file is read in large chunks with read(2) into
//                             a pinned buffer and parsed by kernels (mgx_parse_reads) — file bytes in, TSV bytes out, no per-read
//                             host work.  Files inside the parser's grammar print the same bytes, with two exceptions
//                             where the parser follows kseq and read_records does not: a record with an empty name is printed
//                             (read_records drops it), and in a CRLF file the '\r' is not part of the sequence (std::getline
//                             keeps it).  Files outside the grammar: exit status 1 and the byte position.  Not with --map or
//                             --rccl-gather (--map has --map-on-device, below, which takes --parse-on-device without
//                             --format-on-device)
//             [--load-on-device]  GRAPH.dbg is decoded by kernels (mgx_graph_load_dbg_device): the host walks the file's headers, the
//                             rrr blocks, the wavelet tree of W and `last` are decoded on the device.  The same graph, the same
//                             output; the default decodes on the host (mgx_boss_file_read).  With -a X.column.annodbg the
//                             annotation's columns are decoded by kernels as well (mgx_annotation_load_columns_device) on the
//                             device of the one annotation replica (-a goes with --devices 1); the same output
//             [--devices D]   in-process multi-GPU: one graph replica per device, whole batches routed round-robin, no collective
//             [--rccl-gather] with --devices D: one worker per device, batches in rounds of D; every round's device results are
//                             gathered to device 0 over RCCL (mgx_gather_*: the C-ABI of north_star's "RCCL-over-xGMI only to
//                             gather alignment results"), decoded there (mgx_results_from_raw) and printed by that worker alone
//             [-a ANNOTATION]  label-aware alignment (metagraph align -a: LabeledAligner); every alignment is printed with its
//                              labels' names (cli/align.cpp:274-281).  ANNOTATION: `.column.annodbg` files written by the
//                              reference (-a may be repeated: their columns side by side, mgx_column_file_read), or a dump of
//                              the columns — u64 n_rows, u64 n_labels, then per label: u64 name length, the name, u64 count,
//                              count x u64 rows (row = node - 1)
//                             (the reference's unit of parallelism, cli/align.cpp:440-475: one task per batch)
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <mutex>
#include <thread>

#include <fcntl.h>
#include <unistd.h>

#include "hip_dbg_aligner.hpp"

using namespace mgx::host;

static bool read_records(const std::string &path, std::vector<IDBGAligner::Query> *out) {
    std::ifstream in(path);
    if (!in) return false;
    std::string line, name, seq;
    bool fastq = false;
    auto flush = [&]() { if (!name.empty()) out->emplace_back(name, seq); name.clear(); seq.clear(); };
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        if (line[0] == '@' && (name.empty() || fastq)) {       // FASTQ record: 4 lines
            fastq = true;
            flush();
            name = line.substr(1, line.find_first_of(" \t") - 1);
            std::getline(in, seq);
            std::string plus, qual;
            std::getline(in, plus);
            std::getline(in, qual);
            flush();
        } else if (line[0] == '>') {
            flush();
            name = line.substr(1, line.find_first_of(" \t") - 1);
        } else {
            seq += line;
        }
    }
    flush();
    return true;
}

// cli/align.cpp:415-480: records are read into batches of at most `query_batch_size` bases (default 100 MB,
// cli/config/config.hpp:105), every batch is a task of a pool of `-p` workers; a task builds its own aligner over the
// shared read-only graph and prints each query's line under a mutex as it completes (so with -p 1 output is in input
// order, with more workers batches interleave — exactly the reference's behaviour).
int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s GRAPH.boss READS [--align-only-forwards] [--align-min-exact-match X] [--align-min-seed-length N]\n"
                        "          [-p THREADS] [--query-batch-size BASES] [--max-columns N (test hook: small device arena)]\n", argv[0]);
        return 2;
    }
    auto ends_with = [](const std::string &s, const char *suffix) { const size_t n = strlen(suffix); return s.size() >= n && !s.compare(s.size() - n, n, suffix); };
    uint64_t hdr[7];
    std::vector<uint8_t> W, last;
    uint32_t graph_mode = MGX_MODE_BASIC;
    std::unique_ptr<HipGraphSet> loaded;           // --load-on-device: the replicas, made here (k comes from them)
    bool load_on_device = false;
    int load_devices = 1;
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--load-on-device")) load_on_device = true;
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) load_devices = std::max(1, atoi(argv[++i]));
    }
    if (load_on_device) {
        if (!ends_with(argv[1], ".dbg")) { fprintf(stderr, "error: --load-on-device decodes a `.dbg` file on the device: %s is none\n", argv[1]); return 1; }
        if (load_devices > mgx_device_count() && mgx_device_count() > 0) {
            fprintf(stderr, "error: --devices %d but %d HIP device(s) visible\n", load_devices, mgx_device_count());
            return 1;
        }
        try {
            loaded.reset(new HipGraphSet(load_devices, argv[1], true));
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
        hdr[0] = loaded->for_worker(0).get_k();
        hdr[1] = mgx_graph_num_edges(loaded->for_worker(0).handle());
    } else if (ends_with(argv[1], ".dbg")) {      // DBGSuccinct::load (dbg_succinct.cpp:690-711)
        mgx_boss_file f;
        if (mgx_boss_file_read(argv[1], &f) != MGX_OK) { fprintf(stderr, "error: %s\n", mgx_last_error()); return 1; }
        if (f.sigma != 5) { fprintf(stderr, "error: %s: alphabet of %u characters; DNA graphs only\n", argv[1], f.sigma); mgx_boss_file_free(&f); return 1; }
        hdr[0] = f.k; hdr[1] = f.n_edges;
        for (int i = 0; i < 5; ++i) hdr[2 + i] = f.F[i];
        W.assign(f.W, f.W + f.n_edges + 1);
        last.assign(f.last, f.last + f.n_edges + 1);
        graph_mode = f.mode;
        mgx_boss_file_free(&f);
    } else {
        std::ifstream gin(argv[1], std::ios::binary);
        if (!gin) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
        gin.read((char *)hdr, sizeof(hdr));       // k, n_edges, F[0..4]
        W.resize(hdr[1] + 1); last.resize(hdr[1] + 1);
        gin.read((char *)W.data(), (std::streamsize)W.size());
        gin.read((char *)last.data(), (std::streamsize)last.size());
        if (!gin) { fprintf(stderr, "bad BOSS dump %s\n", argv[1]); return 1; }
    }
    const uint32_t k = (uint32_t)hdr[0];
    const uint64_t n = hdr[1];
    DBGAlignerConfig cfg;
    mgx_config_init_cli(&cfg, k);
    unsigned threads = 1;
    bool report_time = false;
    uint64_t batch_size = 100000000ull;
    mgx_limits lim;
    bool have_lim = false;
    int devices = 1;
    bool rccl_gather = false, format_on_device = false, parse_on_device = false, map_on_device = false;
    bool json = false, have_json_slice_bytes = false;
    uint64_t json_slice_bytes = 256ull << 20;          // --json-slice-bytes N: the estimated text of one mgx_format_json_batch call
    uint64_t parse_chunk_bytes = 256ull << 20;         // --parse-chunk-bytes N (test hook: several chunks from a small file)
    std::vector<const char *> anno_paths;
    std::vector<std::string> kernel_options;            // --kernel-option key=value: result-preserving kernel selection (A/B runs)
    bool map_mode = false, count_kmers = false, query_presence = false, filter_present = false, fwd_and_reverse = false;
    double discovery_fraction = 0.7;                     // cli/config/config.hpp:136
    uint32_t align_length = 0;
    mgx_limits_init_default(&lim, 0);
    for (int i = 3; i < argc; ++i) {
        if (!strcmp(argv[i], "--map")) { map_mode = true; continue; }
        if (!strcmp(argv[i], "--count-kmers")) { count_kmers = true; continue; }
        if (!strcmp(argv[i], "--query-presence")) { query_presence = true; continue; }
        if (!strcmp(argv[i], "--filter-present")) { filter_present = true; continue; }
        if (!strcmp(argv[i], "--fwd-and-reverse")) { fwd_and_reverse = true; continue; }
        if (!strcmp(argv[i], "--discovery-fraction") && i + 1 < argc) { discovery_fraction = atof(argv[++i]); continue; }
        if (!strcmp(argv[i], "--align-length") && i + 1 < argc) { align_length = (uint32_t)std::max(0, atoi(argv[++i])); continue; }
        if (!strcmp(argv[i], "--align-only-forwards")) cfg.forward_and_reverse_complement = 0;
        else if (!strcmp(argv[i], "--align-min-exact-match") && i + 1 < argc) cfg.min_exact_match = atof(argv[++i]);
        else if (!strcmp(argv[i], "--align-min-seed-length") && i + 1 < argc) cfg.min_seed_length = std::min<uint64_t>(atoi(argv[++i]), k);
        else if (!strcmp(argv[i], "-p") && i + 1 < argc) threads = (unsigned)std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--query-batch-size") && i + 1 < argc) batch_size = strtoull(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--max-columns") && i + 1 < argc) { lim.max_columns = (uint32_t)atoi(argv[++i]); have_lim = true; }
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) devices = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "-a") && i + 1 < argc) anno_paths.push_back(argv[++i]);
        else if (!strcmp(argv[i], "--kernel-option") && i + 1 < argc) kernel_options.push_back(argv[++i]);
        else if (!strcmp(argv[i], "--rccl-gather")) rccl_gather = true;
        else if (!strcmp(argv[i], "--format-on-device")) format_on_device = true;
        else if (!strcmp(argv[i], "--parse-on-device")) parse_on_device = true;
        else if (!strcmp(argv[i], "--json")) json = true;
        else if (!strcmp(argv[i], "--json-slice-bytes") && i + 1 < argc) { json_slice_bytes = std::max<uint64_t>(1, strtoull(argv[++i], nullptr, 10)); have_json_slice_bytes = true; }
        else if (!strcmp(argv[i], "--map-on-device")) map_on_device = true;
        else if (!strcmp(argv[i], "--parse-chunk-bytes") && i + 1 < argc) parse_chunk_bytes = std::max<uint64_t>(1, strtoull(argv[++i], nullptr, 10));
        else if (!strcmp(argv[i], "--time")) report_time = true;            // wall time of the align loop (batches -> results printed) on stderr
        else if (!strcmp(argv[i], "--canonical")) graph_mode = MGX_MODE_CANONICAL;
        else if (!strcmp(argv[i], "--primary")) graph_mode = MGX_MODE_PRIMARY;         // aligned through the CanonicalDBG wrapper
    }
    if (map_on_device && !map_mode) {
        fprintf(stderr, "error: --map-on-device writes the text of --map on the device: it needs --map\n");
        return 1;
    }
    // --map --map-on-device --parse-on-device: the parser's device arrays go to one mapper and its formatter
    const bool map_parse_on_device = map_mode && map_on_device && parse_on_device && !format_on_device;
    if (map_parse_on_device && (fwd_and_reverse || threads != 1 || devices != 1)) {
        fprintf(stderr, "error: --map-on-device --parse-on-device maps the parser's device arrays on one device: %s\n",
                fwd_and_reverse ? "not with --fwd-and-reverse (its records are made on the host)" : threads != 1 ? "with -p 1 only" : "with --devices 1 only");
        return 1;
    }
    if (parse_on_device && !map_parse_on_device && (map_mode || rccl_gather || !format_on_device || threads != 1 || devices != 1)) {
        fprintf(stderr, "error: --parse-on-device hands the parser's device arrays to one aligner and its formatter: %s\n",
                map_mode ? "not with --map" : rccl_gather ? "not with --rccl-gather" : !format_on_device ? "it needs --format-on-device"
                : "with -p 1 and --devices 1 only");
        return 1;
    }
    if (format_on_device && (map_mode || rccl_gather)) {
        fprintf(stderr, "error: --format-on-device formats the alignment TSV of a batch on its own device: not with %s\n", map_mode ? "--map" : "--rccl-gather");
        return 1;
    }
    if (json && (map_mode || rccl_gather || cfg.post_chain_alignments)) {
        fprintf(stderr, "error: --json prints the alignments of a batch from its own device: not with %s\n",
                map_mode ? "--map" : rccl_gather ? "--rccl-gather" : "post_chain_alignments (the reference has no JSON output for chains)");
        return 1;
    }
    if (have_json_slice_bytes && !(json && format_on_device)) {
        fprintf(stderr, "error: --json-slice-bytes bounds the text of one mgx_format_json_batch call: it needs --json --format-on-device\n");
        return 1;
    }
    // the end of the --json slice that starts at query `first` of a batch of n: see --json-slice-bytes
    const uint64_t json_paths = std::max<uint64_t>(1, cfg.num_alternative_paths);
    auto json_slice_end = [&](uint64_t first, uint64_t n, auto &&query_len, auto &&header_len) {
        uint64_t end = first, estimate = 0;
        while (end < n) {
            estimate += (128 * (uint64_t)query_len(end) + 2 * (uint64_t)header_len(end) + 512) * json_paths;
            if (end > first && estimate > json_slice_bytes) break;
            ++end;
        }
        return end;
    };
    if (map_mode) anno_paths.clear();                    // no annotation is loaded in this mode (cli/align.cpp:316-318)
    try {
        // one replica of the index per device (3.5 B/edge + the suffix-range table each); more devices than the box shows is an
        // error of the caller's, reported like any other
        if (devices > mgx_device_count() && mgx_device_count() > 0) {
            fprintf(stderr, "error: --devices %d but %d HIP device(s) visible\n", devices, mgx_device_count());
            return 1;
        }
        if (!loaded) loaded.reset(new HipGraphSet(devices, k, n, W.data(), last.data(), hdr + 2, nullptr, graph_mode));
        HipGraphSet &graphs = *loaded;
        std::unique_ptr<HipAnnotation> annotation;
        std::vector<std::string> label_names;
        if (!anno_paths.empty() && devices != 1) { fprintf(stderr, "error: -a with --devices 1 only (one annotation replica)\n"); return 1; }
        if (!anno_paths.empty() && ends_with(anno_paths[0], ".annodbg") && load_on_device) {      // ... with the columns decoded by kernels
            uint64_t n_rows = 0;
            try {
                annotation = std::make_unique<HipAnnotation>(anno_paths, 0, &n_rows, &label_names);
            } catch (const std::runtime_error &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
            if (n_rows != n) { fprintf(stderr, "error: the annotation has %llu rows, the graph %llu nodes\n", (unsigned long long)n_rows, (unsigned long long)n); return 1; }
        } else if (!anno_paths.empty() && ends_with(anno_paths[0], ".annodbg")) {      // ColumnCompressed::merge_load
            mgx_column_file *cf = nullptr;
            if (mgx_column_file_read(anno_paths.data(), (uint32_t)anno_paths.size(), &cf) != MGX_OK) { fprintf(stderr, "error: %s\n", mgx_last_error()); return 1; }
            const uint32_t nl = mgx_column_file_num_labels(cf);
            for (uint32_t j = 0; j < nl; ++j) label_names.emplace_back(mgx_column_file_label(cf, j));
            const uint64_t *cb = mgx_column_file_col_begin(cf), *rw = mgx_column_file_rows(cf);
            const uint64_t n_rows = mgx_column_file_num_rows(cf);
            std::vector<uint64_t> col_begin(cb, cb + nl + 1), rows(rw, rw + cb[nl]);
            mgx_column_file_free(cf);
            // AnnotatedDBG::check_compatibility (annotated_dbg.cpp): one row per node
            if (n_rows != n) { fprintf(stderr, "error: the annotation has %llu rows, the graph %llu nodes\n", (unsigned long long)n_rows, (unsigned long long)n); return 1; }
            annotation = std::make_unique<HipAnnotation>(n_rows, col_begin, rows, 0);
        } else if (!anno_paths.empty()) {
            const char *anno_path = anno_paths[0];
            std::ifstream ain(anno_path, std::ios::binary);
            if (!ain) { fprintf(stderr, "cannot open %s\n", anno_path); return 1; }
            uint64_t n_rows = 0, n_labels = 0;
            ain.read((char *)&n_rows, 8); ain.read((char *)&n_labels, 8);
            std::vector<uint64_t> col_begin{ 0 }, rows;
            for (uint64_t j = 0; j < n_labels && ain; ++j) {
                uint64_t len = 0, cnt = 0;
                ain.read((char *)&len, 8);
                std::string name(len, '\0');
                ain.read(name.data(), (std::streamsize)len);
                ain.read((char *)&cnt, 8);
                const size_t at = rows.size();
                rows.resize(at + cnt);
                ain.read((char *)(rows.data() + at), (std::streamsize)(cnt * 8));
                col_begin.push_back(rows.size());
                label_names.push_back(std::move(name));
            }
            if (!ain || col_begin.size() != n_labels + 1) { fprintf(stderr, "bad annotation dump %s\n", anno_path); return 1; }
            annotation = std::make_unique<HipAnnotation>(n_rows, col_begin, rows, 0);
        }
        if ((unsigned)devices > threads) threads = (unsigned)devices;                  // at least one worker per device
        if (map_mode) {
            // cli/align.cpp:351-355
            if (align_length > k) { fprintf(stderr, "warning: Mapping to k-mers longer than k is not supported. Setting --align-length to %u\n", k); align_length = k; }
            if (!align_length) align_length = k;
        }
        const int map_format = query_presence ? (filter_present ? MGX_MAP_FMT_FILTER_PRESENT : MGX_MAP_FMT_QUERY_PRESENCE)
                               : count_kmers ? MGX_MAP_FMT_COUNT_KMERS : MGX_MAP_FMT_NODES;
        if (parse_on_device) {
            // file bytes in, TSV bytes out: read(2) into a pinned buffer, a parse per chunk (the unconsumed tail is carried over to
            // the next chunk), batches cut at the reference's rule from the parser's host copy of the offsets, aligned from
            // its device arrays, printed from the formatter's text
            const int fd = open(argv[2], O_RDONLY);
            if (fd < 0) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
            struct Pinned {
                char *p = nullptr; size_t cap = 0;
                ~Pinned() { mgx_pinned_free(p); }
                void grow(size_t want, size_t keep) {
                    if (want <= cap) return;
                    void *q = mgx_pinned_alloc(want);
                    if (!q) throw std::runtime_error(std::string("the read buffer: ") + mgx_last_error());
                    if (keep) memcpy(q, p, keep);
                    mgx_pinned_free(p);
                    p = static_cast<char *>(q); cap = want;
                }
            } buf;
            parse_chunk_bytes = std::min<uint64_t>(parse_chunk_bytes, 0xF0000000ull);
            const HipBOSSGraph &graph = graphs.for_worker(0);
            HipReadParser parser(0);
            std::unique_ptr<HipGraphMapper> mapper;
            if (map_mode) {
                mapper.reset(new HipGraphMapper(graph));
                for (const std::string &opt : kernel_options) mapper->set_kernel_option(opt);
            }
            const auto t0 = std::chrono::steady_clock::now();
            size_t have = 0, n_queries = 0, n_batches = 0;
            uint64_t file_at = 0;                      // the file position of buf[0]
            uint32_t format = 0;
            bool eof = false;
            int status = 0;
            while (!eof || have) {
                // fill: one more chunk behind what the last parse left
                buf.grow(have + parse_chunk_bytes, have);
                while (!eof && have < buf.cap) {
                    const ssize_t got = read(fd, buf.p + have, std::min<size_t>(buf.cap - have, parse_chunk_bytes));
                    if (got < 0) { fprintf(stderr, "error: reading %s failed\n", argv[2]); close(fd); return 1; }
                    if (got == 0) eof = true; else have += (size_t)got;
                    if (have >= parse_chunk_bytes) break;
                }
                if (have >= 0xFFFFFFF0ull) { fprintf(stderr, "error: a record of %s does not fit a chunk of 4 GB; run without --parse-on-device\n", argv[2]); status = 1; break; }
                mgx_reads r;
                try { r = parser.parse(buf.p, have, eof, format); }
                catch (const ParseRefused &e) {
                    fprintf(stderr, "error: %s: %s (positions count from byte %llu of the file); run without --parse-on-device\n", argv[2], e.what(), (unsigned long long)file_at);
                    status = 1;
                    break;
                }
                if (!format) format = r.format;
                for (uint64_t i = 0; i < r.n_records;) {
                    // align.cpp:431-442: a record is added while the running total is <= batch_size
                    const uint64_t first = i;
                    while (i < r.n_records && r.host_offsets[i] - r.host_offsets[first] <= batch_size) ++i;
                    const char *d_seqs; const uint64_t *d_offsets;
                    parser.slice(first, i - first, &d_seqs, &d_offsets);
                    if (map_mode) {
                        mapper->map_batch_device(d_seqs, d_offsets, i - first, align_length, map_format == MGX_MAP_FMT_NODES);
                        const std::string_view text = mapper->format_batch(r.names, r.name_offsets + first, i - first, map_format, discovery_fraction);
                        std::cout.write(text.data(), (std::streamsize)text.size());
                        ++n_batches;
                        continue;
                    }
                    std::unique_ptr<HipDBGAligner> aligner_p(annotation
                        ? new HipDBGAligner(graph, cfg, *annotation, have_lim ? &lim : nullptr)
                        : new HipDBGAligner(graph, cfg, have_lim ? &lim : nullptr));
                    for (const std::string &opt : kernel_options) aligner_p->set_kernel_option(opt);
                    aligner_p->align_batch_device(d_seqs, d_offsets, i - first);
                    if (json) {
                        const uint64_t nb = i - first, *ho = r.host_offsets + first, *no = r.name_offsets + first;
                        for (uint64_t at = 0; at < nb;) {
                            const uint64_t end = json_slice_end(at, nb, [&](uint64_t t) { return ho[t + 1] - ho[t]; }, [&](uint64_t t) { return no[t + 1] - no[t]; });
                            const std::string_view text = aligner_p->format_batch_json(r.names, no, at, end - at);
                            std::cout.write(text.data(), (std::streamsize)text.size());
                            at = end;
                        }
                        ++n_batches;
                        continue;
                    }
                    const std::string_view text = aligner_p->format_batch_tsv(r.names, r.name_offsets + first, i - first, annotation ? &label_names : nullptr);
                    std::cout.write(text.data(), (std::streamsize)text.size());
                    ++n_batches;
                }
                n_queries += r.n_records;
                memmove(buf.p, buf.p + r.consumed, have - r.consumed);
                have -= r.consumed;
                file_at += r.consumed;
                if (eof) break;
            }
            close(fd);
            std::cout.flush();
            if (report_time && !status) {
                const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                fprintf(stderr, "mgx_align: %zu queries in %zu batches, 1 worker(s), %.3f s in the read-parse-%s loop (%.0f queries/s)\n",
                        n_queries, n_batches, sec, map_mode ? "map" : "align", sec > 0 ? (double)n_queries / sec : 0.0);
            }
            return status;
        }
        std::vector<IDBGAligner::Query> all;
        if (!read_records(argv[2], &all)) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
        if (map_mode) {
            if (fwd_and_reverse) {                      // sequence_io.hpp:317-319
                std::vector<IDBGAligner::Query> both;
                for (auto &q : all) {
                    std::string rc(q.second.rbegin(), q.second.rend());
                    for (char &c : rc)
                        switch (c) {
                            case 'A': c = 'T'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break; case 'T': c = 'A'; break;
                            case 'a': c = 't'; break; case 'c': c = 'g'; break; case 'g': c = 'c'; break; case 't': c = 'a'; break;
                            default: break;
                        }
                    both.push_back(q);
                    both.emplace_back(q.first, std::move(rc));
                }
                all.swap(both);
            }
            const int format = map_format;
            HipGraphMapper mapper(graphs.for_worker(0));
            for (const std::string &opt : kernel_options) mapper.set_kernel_option(opt);
            std::string line;
            for (size_t i = 0; i < all.size();) {
                const size_t first = i;
                std::vector<std::string_view> seqs;
                uint64_t bytes = 0;
                for (; i < all.size() && bytes <= batch_size; ++i) { bytes += all[i].second.size(); seqs.emplace_back(all[i].second); }
                if (map_on_device) {
                    // the node array stays in device memory; the text of the whole batch comes back in one piece
                    mapper.map_batch(seqs, align_length, false, format == MGX_MAP_FMT_NODES);
                    std::string names;
                    std::vector<uint64_t> name_offsets(seqs.size() + 1, 0);
                    for (size_t t = 0; t < seqs.size(); ++t) { names += all[first + t].first.c_str(); name_offsets[t + 1] = names.size(); }
                    const std::string_view text = mapper.format_batch(names.data(), name_offsets.data(), seqs.size(), format, discovery_fraction);
                    std::cout.write(text.data(), (std::streamsize)text.size());
                    continue;
                }
                const mgx_map_summary s = mapper.map_batch(seqs, align_length, format == MGX_MAP_FMT_NODES);
                for (size_t t = 0; t < seqs.size(); ++t) {
                    const IDBGAligner::Query &q = all[first + t];
                    const size_t need = mgx_format_map(&s, t, q.first.c_str(), q.second.data(), q.second.size(), k, align_length, format,
                                                       discovery_fraction, nullptr, 0);
                    line.resize(need + 1);
                    mgx_format_map(&s, t, q.first.c_str(), q.second.data(), q.second.size(), k, align_length, format, discovery_fraction,
                                   line.data(), need + 1);
                    std::cout.write(line.data(), (std::streamsize)need);
                }
            }
            std::cout.flush();
            return 0;
        }
        // batches by bases read (align.cpp:431-442: a record is added while the running total is <= batch_size)
        std::vector<std::vector<IDBGAligner::Query>> batches;
        const size_t n_queries = all.size();
        for (size_t i = 0; i < all.size();) {
            std::vector<IDBGAligner::Query> b;
            uint64_t bytes = 0;
            for (; i < all.size() && bytes <= batch_size; ++i) { bytes += all[i].second.size(); b.push_back(std::move(all[i])); }
            batches.push_back(std::move(b));
        }
        std::mutex print_mutex, err_mutex;
        std::atomic<size_t> next{ 0 };
        std::string first_error;
        auto worker = [&](unsigned worker_id) {
            try {
                const HipBOSSGraph &graph = graphs.for_worker(worker_id);               // a worker stays on its device
                for (;;) {
                    const size_t bi = next.fetch_add(1);
                    if (bi >= batches.size()) break;
                    // one aligner per task, shared graph (and annotation: LabeledAligner<>(graph, config, annotator))
                    std::unique_ptr<HipDBGAligner> aligner_p(annotation
                        ? new HipDBGAligner(graph, cfg, *annotation, have_lim ? &lim : nullptr)
                        : new HipDBGAligner(graph, cfg, have_lim ? &lim : nullptr));
                    HipDBGAligner &aligner = *aligner_p;
                    // (the workers of one device share it: every handle on its own stream, its arenas sized for its share)
                    aligner.set_device_share((threads + (unsigned)devices - 1) / (unsigned)devices);
                    for (const std::string &opt : kernel_options) aligner.set_kernel_option(opt);
                    if (json) {
                        const std::vector<IDBGAligner::Query> &batch = batches[bi];
                        aligner.align_batch_device(batch);
                        std::lock_guard<std::mutex> lock(print_mutex);          // (a batch's lines stay together)
                        if (format_on_device) {
                            for (uint64_t at = 0; at < batch.size();) {
                                const uint64_t end = json_slice_end(at, batch.size(), [&](uint64_t t) { return batch[t].second.size(); },
                                                                    [&](uint64_t t) { return batch[t].first.size(); });
                                const std::string_view text = aligner.format_batch_json(batch, at, end - at);
                                std::cout.write(text.data(), (std::streamsize)text.size());
                                at = end;
                            }
                            continue;
                        }
                        mgx_results res{};
                        if (int rc = mgx_fetch_results(aligner.handle(), &res))
                            throw std::runtime_error(std::string("mgx_fetch_results: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
                        std::string line;
                        for (size_t t = 0; t < batch.size(); ++t) {
                            if (res.status[t] != MGX_OK)
                                throw std::runtime_error("query " + std::to_string(t) + " (" + batch[t].first + "): status " + std::to_string(res.status[t]));
                            const size_t need = mgx_format_json(&res, t, batch[t].first.c_str(), batch[t].second.data(), batch[t].second.size(), k, nullptr, 0);
                            line.resize(need + 1);
                            mgx_format_json(&res, t, batch[t].first.c_str(), batch[t].second.data(), batch[t].second.size(), k, line.data(), need + 1);
                            std::cout.write(line.data(), (std::streamsize)need);
                        }
                        continue;
                    }
                    if (format_on_device) {
                        aligner.align_batch_device(batches[bi]);
                        const std::string_view text = aligner.format_batch_tsv(batches[bi], annotation ? &label_names : nullptr);
                        std::lock_guard<std::mutex> lock(print_mutex);
                        std::cout.write(text.data(), (std::streamsize)text.size());
                        continue;
                    }
                    aligner.align_batch(batches[bi], [&](const std::string &header, AlignmentResults &&paths) {
                        const std::string res = format_alignment(header, paths, cfg.min_path_score, annotation ? &label_names : nullptr);
                        std::lock_guard<std::mutex> lock(print_mutex);
                        std::cout << res;
                    });
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lock(err_mutex);
                if (first_error.empty()) first_error = e.what();
            }
        };
        // --rccl-gather: worker w = rank w = device w; round r takes batches r D .. r D + D - 1 (a rank without one aligns an empty
        // batch: the gather is collective); rank 0 receives every rank's records and stream and prints the round
        std::vector<mgx_gather *> gathers((size_t)devices, nullptr);
        auto gather_worker = [&](unsigned w) {
            const size_t D = (size_t)devices, rounds = (batches.size() + D - 1) / D;
            const HipBOSSGraph &graph = graphs.for_worker(w);
            static const std::vector<IDBGAligner::Query> no_queries;
            for (size_t r = 0; r < rounds; ++r) {
                const size_t bi = r * D + w;
                const std::vector<IDBGAligner::Query> &mine = bi < batches.size() ? batches[bi] : no_queries;
                std::unique_ptr<HipDBGAligner> aligner_p;
                bool ok = true;
                try {
                    aligner_p.reset(annotation ? new HipDBGAligner(graph, cfg, *annotation, have_lim ? &lim : nullptr)
                                               : new HipDBGAligner(graph, cfg, have_lim ? &lim : nullptr));
                    for (const std::string &opt : kernel_options) aligner_p->set_kernel_option(opt);
                    aligner_p->align_batch_device(mine);
                } catch (const std::exception &e) {
                    std::lock_guard<std::mutex> lock(err_mutex);
                    if (first_error.empty()) first_error = e.what();
                    ok = false;
                }
                if (!ok) {                            // (stay in the collective: the other ranks are waiting in it)
                    try { aligner_p.reset(new HipDBGAligner(graph, cfg, have_lim ? &lim : nullptr)); aligner_p->align_batch_device(no_queries); }
                    catch (const std::exception &) { fprintf(stderr, "error: rank %u cannot take part in the gather\n", w); std::abort(); }
                }
                std::vector<uint64_t> nq(D), words(D);
                std::vector<const void *> hdrs(D);
                std::vector<const uint32_t *> streams(D);
                if (mgx_gather_start(gathers[w], aligner_p->handle()) != MGX_OK
                    || mgx_gather_finish(gathers[w], nq.data(), hdrs.data(), streams.data(), words.data()) != MGX_OK) {
                    fprintf(stderr, "error: rank %u: %s\n", w, mgx_last_error());
                    std::abort();                    // (a broken collective cannot be left politely)
                }
                if (w != 0) continue;
                for (size_t q = 0; q < D; ++q) {
                    const size_t bq = r * D + q;
                    if (bq >= batches.size()) continue;
                    try {
                        if (nq[q] != batches[bq].size()) throw std::runtime_error("rank " + std::to_string(q) + " sent " + std::to_string(nq[q]) + " records for a batch of " + std::to_string(batches[bq].size()));
                        mgx_raw_store *store = nullptr;
                        mgx_results res{};
                        if (int rc = mgx_results_from_raw_labeled(hdrs[q], nq[q], streams[q], words[q], annotation ? 1 : 0, &store, &res))
                            throw std::runtime_error(std::string("mgx_results_from_raw: ") + mgx_last_error() + " (" + std::to_string(rc) + ")");
                        try {
                            HipDBGAligner::deliver(res, batches[bq], [&](const std::string &header, AlignmentResults &&paths) {
                                std::cout << format_alignment(header, paths, cfg.min_path_score, annotation ? &label_names : nullptr);
                            });
                        } catch (...) { mgx_raw_store_free(store); throw; }
                        mgx_raw_store_free(store);
                    } catch (const std::exception &e) {
                        std::lock_guard<std::mutex> lock(err_mutex);
                        if (first_error.empty()) first_error = e.what();
                    }
                }
            }
        };
        if (rccl_gather) {
            std::vector<int> devs((size_t)devices);
            for (int d = 0; d < devices; ++d) devs[(size_t)d] = d;
            if (int rc = mgx_gather_create_local(devs.data(), devices, 0, gathers.data())) {
                fprintf(stderr, "error: %s (%d)\n", mgx_last_error(), rc);
                return 1;
            }
            threads = (unsigned)devices;
        }
        const auto t_align0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        if (rccl_gather) {
            for (unsigned t = 1; t < threads; ++t) pool.emplace_back(gather_worker, t);
            gather_worker(0);
        } else {
            for (unsigned t = 1; t < threads; ++t) pool.emplace_back(worker, t);
            worker(0);
        }
        for (auto &t : pool) t.join();
        for (mgx_gather *g : gathers) mgx_gather_destroy(g);
        if (report_time) {
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_align0).count();
            fprintf(stderr, "mgx_align: %zu queries in %zu batches, %u worker(s), %.3f s in the align loop (%.0f queries/s)\n",
                    n_queries, batches.size(), threads, sec, sec > 0 ? (double)n_queries / sec : 0.0);
        }
        if (!first_error.empty()) { fprintf(stderr, "error: %s\n", first_error.c_str()); return 1; }
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
