// tests/emu/reads_parse_check.cpp — TEST ONLY: metagraph_amd/csrc/reads_parse.hpp (the passes of mgx_parse_reads) under the host
// wave model.  tests/test_reads_parse_model.py writes the cases and compares what comes back with its restatement of the grammar.
// usage: reads_parse_check <cases> <results>
//   case:   u64 n_bytes, u32 flags, u32 mis (the text's address & 15), u32 n_sizes, u32 0, u64 sizes[n_sizes], text
//           the text is fed in chunks: the buffer grows by sizes[k] (cyclic) per call and shrinks by what the call consumed;
//           the call that reaches the end of the text is the final one
//   result: i64 rc (0, or -1: refused), u64 error position (in the file), u64 n_records, u64 consumed, u64 format, u64 seq bytes,
//           u64 name bytes, u64 calls, offsets[n + 1], name_offsets[n + 1], seqs, names
#include "wave.hpp"
#include "../../metagraph_amd/csrc/reads_parse.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace mgx;

struct Parsed {
    int rc = 0;
    uint64_t err_pos = 0, n_records = 0, consumed = 0;
    uint32_t format = 0;
    std::vector<uint64_t> offsets, name_offsets;
    std::string seqs, names;
};

// one call of mgx_parse_reads, the kernels' lanes one after the other
static Parsed parse(const char *text, uint64_t n, bool final_chunk, uint32_t flags) {
    Parsed out;
    out.offsets.assign(1, 0); out.name_offsets.assign(1, 0);
    uint64_t pos = 0;
    int fmt = rp_detect_format([&](uint64_t p) { return text[p]; }, n, final_chunk, &pos);
    if (fmt < 0) { out.rc = -1; out.err_pos = pos; return out; }
    if (flags) fmt = (int)flags;
    if (fmt == 0) { out.consumed = final_chunk ? n : 0; return out; }
    out.format = (uint32_t)fmt;
    RpChunk c;
    memset(&c, 0, sizeof(c));
    c.text = text; c.n = n; c.mis = (uint32_t)((uintptr_t)text & 15u); c.n_spans = (uint32_t)((n + c.mis + RP_SPAN - 1) / RP_SPAN);
    c.format = (uint32_t)fmt; c.final_chunk = final_chunk ? 1 : 0;
    std::vector<uint64_t> mask(c.n_spans);
    std::vector<uint32_t> span_count(c.n_spans + 1, 0), span_first(c.n_spans + 1, 0);
    c.mask = mask.data(); c.span_count = span_count.data(); c.span_first = span_first.data();
    for (uint32_t s = 0; s < c.n_spans; ++s) rp_line_count(c, s);
    for (uint32_t s = 0; s < c.n_spans; ++s) span_first[s + 1] = span_first[s] + span_count[s];
    const uint32_t n_nl = span_first[c.n_spans];
    std::vector<uint32_t> line_begin(n_nl + 2, 0xDEADBEEFu);
    c.line_begin = line_begin.data();
    for (uint32_t s = 0; s < c.n_spans; ++s) rp_line_table(c, s);
    c.n_lines = n_nl + (final_chunk && text[n - 1] != '\n' ? 1u : 0u);
    std::vector<RpSum> items(c.n_lines + 1), sums(c.n_lines + 1);
    RpCounters k;
    memset(&k, 0, sizeof(k));
    k.err_pos = RP_NO_ERROR;
    c.items = items.data(); c.sums = sums.data(); c.ctr = &k;
    for (uint32_t i = 0; i <= c.n_lines; ++i) { const uint32_t v = rp_classify(c, i); if (v > k.last_nonempty) k.last_nonempty = v; }
    RpSum run = { 0, 0, 0 };
    for (uint32_t i = 0; i <= c.n_lines; ++i) { sums[i] = run; run.seq += items[i].seq; run.name += items[i].name; run.rec += items[i].rec; }
    std::vector<uint64_t> offsets(run.rec + 1, ~0ull), name_offsets(run.rec + 1, ~0ull);
    c.offsets = offsets.data(); c.name_offsets = name_offsets.data();
    for (uint32_t i = 0; i <= c.n_lines; ++i) rp_records(c, i);
    if (rp_verdict(c.format, c.n_lines, final_chunk, k, &pos)) { out.rc = -1; out.err_pos = pos; return out; }
    c.seq_bytes = k.seq_bytes; c.name_bytes = k.name_bytes;
    // 16-byte aligned destinations with 16 bytes of room behind them, guarded on both sides
    const char guard = (char)0xA5;
    std::vector<char> sbuf(c.seq_bytes + 64, guard), nbuf(c.name_bytes + 64, guard);
    c.seqs = sbuf.data() + 32 - ((uintptr_t)sbuf.data() & 15u);
    c.names = nbuf.data() + 32 - ((uintptr_t)nbuf.data() & 15u);
    // as k_parse_copy: lanes 0 and 63 of a wavefront bracket the lines of its 64 lanes
    for (uint64_t t0 = 0; 16 * t0 < c.seq_bytes; t0 += 64) {
        const uint32_t lo = rp_wave_line<0>(c, t0, false), hi = rp_wave_line<0>(c, t0, true) + 1;
        for (uint64_t t = t0; t < t0 + 64 && 16 * t < c.seq_bytes; ++t) rp_copy16<0>(c, t, lo, hi);
    }
    for (uint64_t t0 = 0; 16 * t0 < c.name_bytes; t0 += 64) {
        const uint32_t lo = rp_wave_line<1>(c, t0, false), hi = rp_wave_line<1>(c, t0, true) + 1;
        for (uint64_t t = t0; t < t0 + 64 && 16 * t < c.name_bytes; ++t) rp_copy16<1>(c, t, lo, hi);
    }
    if (c.seqs[-1] != guard || c.seqs[c.seq_bytes + 16] != guard || c.names[-1] != guard || c.names[c.name_bytes + 16] != guard) {
        printf("FAIL: a byte outside the destination's room was written\n");
        exit(1);
    }
    out.n_records = k.n_records; out.consumed = final_chunk ? n : k.consumed;
    out.offsets.assign(offsets.begin(), offsets.begin() + k.n_records + 1);
    out.name_offsets.assign(name_offsets.begin(), name_offsets.begin() + k.n_records + 1);
    if (out.offsets.back() != k.seq_bytes || out.name_offsets.back() != k.name_bytes) { printf("FAIL: offsets[n] differs from the byte count\n"); exit(1); }
    out.seqs.assign(c.seqs, c.seq_bytes); out.names.assign(c.names, c.name_bytes);
    return out;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    // the four-byte newline test against the one-byte rule, every byte value in every position
    for (uint32_t ch = 0; ch < 256; ++ch)
        for (int at = 0; at < 4; ++at)
            for (uint32_t others : { 0x0A0A0A0Au, 0x0B090A8Au, 0x00FF8A0Bu }) {
                const uint32_t w = (others & ~(0xFFu << (8 * at))) | (ch << (8 * at));
                uint32_t want = 0;
                for (int x = 0; x < 4; ++x) want |= (uint32_t)(((w >> (8 * x)) & 0xFFu) == '\n') << x;
                if (rp_newlines4(w) != want) { printf("FAIL rp_newlines4(%08x) = %x, want %x\n", w, rp_newlines4(w), want); return 1; }
            }
    FILE *in = fopen(argv[1], "rb"), *outf = fopen(argv[2], "wb");
    if (!in || !outf) return 2;
    uint64_t n_cases = 0;
    for (;;) {
        uint64_t total;
        uint32_t h[4];
        if (fread(&total, 8, 1, in) != 1) break;
        if (fread(h, 4, 4, in) != 4) return 2;
        const uint32_t flags = h[0], mis = h[1] & 15u, n_sizes = h[2];
        std::vector<uint64_t> sizes(n_sizes);
        if (n_sizes == 0 || fread(sizes.data(), 8, n_sizes, in) != n_sizes) return 2;
        std::vector<char> file(total);
        if (total && fread(file.data(), 1, total, in) != total) return 2;
        Parsed all;
        all.offsets.assign(1, 0); all.name_offsets.assign(1, 0);
        uint64_t at = 0, len = 0, calls = 0;
        std::vector<char> buf;
        for (size_t kx = 0;; ++kx) {
            len += sizes[kx % n_sizes];
            const bool final_chunk = at + len >= total;
            if (final_chunk) len = total - at;
            // the chunk at the case's misalignment, other bytes around it
            buf.assign(len + 64, '\n');
            char *text = buf.data() + 16 - ((uintptr_t)buf.data() & 15u) + mis;
            if (len) memcpy(text, file.data() + at, len);
            // (a later chunk is read as what the first one was: the feeder passes the format on)
            const Parsed p = parse(text, len, final_chunk, flags ? flags : all.format);
            ++calls;
            if (p.rc) { all.rc = p.rc; all.err_pos = at + p.err_pos; break; }
            if (!all.format) all.format = p.format;
            for (uint64_t r = 0; r < p.n_records; ++r) {
                all.offsets.push_back(all.offsets[all.n_records] + p.offsets[r + 1]);
                all.name_offsets.push_back(all.name_offsets[all.n_records] + p.name_offsets[r + 1]);
            }
            all.n_records += p.n_records;
            all.seqs += p.seqs; all.names += p.names;
            at += p.consumed; len -= p.consumed;
            if (final_chunk) break;
        }
        all.consumed = at;
        if (all.rc) { all.n_records = 0; all.offsets.assign(1, 0); all.name_offsets.assign(1, 0); all.seqs.clear(); all.names.clear(); }
        const uint64_t head[8] = { (uint64_t)(int64_t)all.rc, all.err_pos, all.n_records, all.consumed, all.format, all.seqs.size(), all.names.size(), calls };
        fwrite(head, 8, 8, outf);
        fwrite(all.offsets.data(), 8, all.offsets.size(), outf);
        fwrite(all.name_offsets.data(), 8, all.name_offsets.size(), outf);
        fwrite(all.seqs.data(), 1, all.seqs.size(), outf);
        fwrite(all.names.data(), 1, all.names.size(), outf);
        ++n_cases;
    }
    fclose(outf);
    printf("ok %llu cases\n", (unsigned long long)n_cases);
    return 0;
}
