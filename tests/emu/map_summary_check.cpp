// tests/emu/map_summary_check.cpp — TEST ONLY: metagraph_amd/csrc/map_summary.hpp under the host wave model against a
// std::set brute force (tests/test_map_summary_model.py builds and runs it).
#include "wave.hpp"
#include "../../metagraph_amd/csrc/map_summary.hpp"

#include <cstdio>
#include <random>
#include <set>
#include <vector>

using namespace mgx;

static uint64_t n_cases = 0;

static bool check(std::mt19937_64 &rng, int mode, int32_t n, uint32_t id_range, int zero_pct, bool masked) {
    const uint32_t n_edges = id_range / 2 + 1;
    std::vector<uint32_t> fwd(n + 1), rc(n + 1);
    auto draw = [&]() -> uint32_t { return (int)(rng() % 100) < zero_pct ? 0u : 1u + (uint32_t)(rng() % id_range); };
    for (int32_t i = 0; i < n; ++i) { fwd[i] = draw(); rc[i] = draw(); }
    std::vector<uint64_t> valid((id_range >> 6) + 2);
    for (auto &w : valid) w = rng() | rng();
    MsRead r = { fwd.data(), rc.data(), n, mode, n_edges, masked ? valid.data() : nullptr };
    // the rules of the issue, restated
    std::vector<uint64_t> want(n);
    for (int32_t i = 0; i < n; ++i) {
        uint64_t v = fwd[i];
        if (mode == MS_MODE_CANONICAL) {
            v = std::min(fwd[i], rc[n - 1 - i]);
            if (masked && !((valid[v >> 6] >> (v & 63)) & 1)) v = 0;
        } else if (mode == MS_MODE_PRIMARY) {
            v = v > n_edges ? v - n_edges : v;
        }
        want[i] = v;
    }
    std::set<uint64_t> distinct;
    uint32_t found = 0;
    for (uint64_t v : want) if (v) { ++found; distinct.insert(v); }
    std::vector<uint32_t> lds(MS_CHUNK), scratch(n + 1);
    for (int form = 0; form < 2; ++form) {
        if (form == 0 && n > MS_SHORT_MAX) continue;
        std::vector<uint64_t> out(n + 1, ~0ull);
        const MsCounts c = form == 0 ? ms_summary_short(r, lds.data(), out.data()) : ms_summary_long(r, lds.data(), scratch.data(), out.data());
        ++n_cases;
        bool ok = c.n_discovered == found && c.n_kmers == (uint32_t)n && c.n_unique == distinct.size() && out[n] == ~0ull;
        for (int32_t i = 0; ok && i < n; ++i) ok = out[i] == want[i];
        // and without the node array
        const MsCounts d = form == 0 ? ms_summary_short(r, lds.data(), nullptr) : ms_summary_long(r, lds.data(), scratch.data(), nullptr);
        ok = ok && d.n_discovered == c.n_discovered && d.n_kmers == c.n_kmers && d.n_unique == c.n_unique;
        if (!ok) {
            printf("FAIL mode %d form %d n %d range %u zeros %d%% masked %d: got %u/%u/%u want %u/%d/%zu\n", mode, form, n, id_range, zero_pct,
                   (int)masked, c.n_discovered, c.n_kmers, c.n_unique, found, n, distinct.size());
            return false;
        }
    }
    return true;
}

int main() {
    std::mt19937_64 rng(20240611);
    const int32_t lengths[] = { 0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 140, 255, 256, 257, 1000, 4095, 4096, 4097, 8192, 8193, 12289, 20000, 32704, 33000 };
    const uint32_t ranges[] = { 1, 3, 40, 5000, 4000000 };        // few ids = many repeats
    for (int mode = 0; mode < 3; ++mode)
        for (int32_t n : lengths)
            for (uint32_t range : ranges)
                for (int zeros : { 0, 30, 95, 100 })
                    for (int masked = 0; masked < (mode == MS_MODE_CANONICAL ? 2 : 1); ++masked)
                        if (!check(rng, mode, n, range, zeros, masked != 0)) return 1;
    for (int it = 0; it < 3000; ++it)
        if (!check(rng, (int)(rng() % 3), (int32_t)(rng() % 700), 1u + (uint32_t)(rng() % 300), (int)(rng() % 101), (rng() & 1) != 0)) return 1;
    printf("ok %llu summaries\n", (unsigned long long)n_cases);
    return 0;
}
