// tools/parse_bench_host.cpp — leg (b) of tools/parse_bench.py: the way to the seqs / offsets arrays before mgx_parse_reads
// existed — the driver's read_records (a std::getline loop, two std::strings per record; copied from mgx_align.cpp as it stands)
// followed by the concatenation HipDBGAligner::align_batch_device does.  Prints one line per run: seconds, records, bases.
// usage: parse_bench_host FILE RUNS
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <utility>
#include <vector>

typedef std::pair<std::string, std::string> Query;

static bool read_records(const std::string &path, std::vector<Query> *out) {
    std::ifstream in(path);
    if (!in) return false;
    std::string line, name, seq;
    bool fastq = false;
    auto flush = [&]() { if (!name.empty()) out->emplace_back(name, seq); name.clear(); seq.clear(); };
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        if (line[0] == '@' && (name.empty() || fastq)) {
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

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    for (int run = 0; run < atoi(argv[2]); ++run) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<Query> all;
        if (!read_records(argv[1], &all)) return 1;
        std::string blob;
        std::vector<unsigned long long> offsets(all.size() + 1, 0);
        for (size_t t = 0; t < all.size(); ++t) { blob += all[t].second; offsets[t + 1] = blob.size(); }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("%.6f %zu %zu\n", sec, all.size(), blob.size());
    }
    return 0;
}
