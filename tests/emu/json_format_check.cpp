// tests/emu/json_format_check.cpp — TEST ONLY: metagraph_amd/csrc/json_format.hpp (the size and the write pass of the batched JSON
// formatter) under the host wave model on generated records.  It dumps records, stream, reads, headers and the text it produced;
// tests/test_json_format_model.py decodes the same records with mgx_results_from_raw_labeled and compares the text with
// mgx_format_json's.  It asserts itself that the batch holds the cases the formatter has to get right (see `Seen`).
// usage: json_format_check <out-prefix>  ->  <out-prefix>.<variant>.bin
//        json_format_check identity      ->  jf_identity against snprintf("%.17g") + the ".0" rule
#include "wave.hpp"
#include "../../metagraph_amd/csrc/json_format.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

using namespace mgx;

template <class T> static void put(FILE *f, const std::vector<T> &v, size_t n) { if (n) fwrite(v.data(), sizeof(T), n, f); }

// what the generated batch must contain
struct Seen {
    bool secondary = false, fwd = false, rev = false, neg_score = false, lead_clip = false, trail_clip = false;
    bool ins_front = false, ins_inside = false, ins_split = false, ins_before_node = false, deletion = false, ends_in_first = false;
    bool offset = false, circular = false, no_seq = false, unmapped = false, many_runs = false, empty_query = false;
    bool esc_mismatch[2] = { false, false }, esc_insertion[2] = { false, false }, node_1_digit = false, node_10_digits = false;
    bool no_alignment = false, capacity = false, hdr_empty = false, hdr_long = false;
    std::set<uint32_t> n_nodes;
};

#define NEED(c) do { if (!(c)) { printf("FAIL: the batch lacks: %s\n", #c); return false; } } while (0)

static bool variant(const std::string &path, uint64_t seed, bool labeled, uint32_t k) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    Seen seen;
    const uint64_t n = 260;
    std::vector<ReadResult> rec(n);
    std::vector<uint32_t> stream;
    std::vector<uint64_t> offsets(1, 0), hoff(1, 0);
    std::string seqs, headers;
    // lower case, N, IUPAC, bytes >= 0x80, '"', '\\', control bytes, 0x7F
    static const char qchars[] = "ACGTACGTACGTacgtNnRYKMSWBDHVrykm\x80\xff\xc3\xe9\x7f\"\\\x01\x08\x09\x0a\x0c\x0d\x1f@[`{~ 09";
    static const char hchars[] = "abcXYZ019 _/|:\"\\\t\x01\x7f\xe9\xc3\x0a";
    const uint64_t cap_query = 137;
    auto node_id = [&]() -> uint32_t {
        const int c = (int)rnd(4);
        const uint32_t v = c == 0 ? (uint32_t)rnd(10) : c == 1 ? 1000000000u + (uint32_t)rnd(3294967295u) : (uint32_t)rnd(5000000);
        if (v < 10) seen.node_1_digit = true;
        if (v >= 1000000000u) seen.node_10_digits = true;
        return v;
    };
    // plain paths of exactly these many nodes: query of nodes - 1 + k characters, offset 0, no indels
    static const uint32_t exact_nodes[] = { 1, 2, 63, 64, 65, 130, 200 };
    for (uint64_t q = 0; q < n; ++q) {
        const bool exact = q >= 20 && q < 27;
        uint32_t qlen = q % 29 == 3 ? 0 : (uint32_t)rnd(q % 7 == 0 ? 700 : 180);
        if (exact) qlen = exact_nodes[q - 20] - 1 + k;
        const uint64_t sb = seqs.size();
        for (uint32_t i = 0; i < qlen; ++i) seqs += qchars[rnd(sizeof(qchars) - 1)];
        offsets.push_back(seqs.size());
        const uint32_t hlen = q % 11 == 0 ? 0 : q % 13 == 0 ? 1000 : (uint32_t)rnd(40);
        for (uint32_t i = 0; i < hlen; ++i) headers += hchars[rnd(sizeof(hchars) - 1)];
        hoff.push_back(headers.size());
        ReadResult &r = rec[q];
        memset(&r, 0, sizeof(r));
        r.n_alignments = (int32_t)rnd(5);
        if (exact) r.n_alignments = 1;
        r.status = ST_OK;
        if (q == cap_query) { r.status = ST_CAPACITY; r.n_alignments = 2; seen.capacity = true; }      // (what it points to is never read)
        r.stream_off = stream.size();
        if (r.status != ST_OK) continue;
        if (hlen == 0) seen.hdr_empty = true;
        if (hlen == 1000) seen.hdr_long = true;
        if (qlen == 0) seen.empty_query = true;
        if (r.n_alignments == 0) seen.no_alignment = true;
        if (r.n_alignments > 1) seen.secondary = true;
        for (int32_t a = 0; a < r.n_alignments; ++a) {
            const int32_t score = (int32_t)rnd(7) == 0 ? -(int32_t)rnd(100000) - 1 : (int32_t)rnd(3000);
            const uint32_t orientation = (uint32_t)rnd(2);
            uint32_t offset = (uint32_t)rnd(3) ? 0 : (uint32_t)rnd(k);
            const JfStrand strand = { seqs.data() + sb, qlen, orientation };
            // a CIGAR over the query: clips, then runs that take exactly the characters between them
            std::vector<uint32_t> cigar;
            uint32_t lead = 0, trail = 0;
            if (!exact && qlen && rnd(3) == 0) lead = (uint32_t)rnd(qlen < 12 ? qlen + 1 : 12);
            if (!exact && qlen > lead && rnd(3) == 0) trail = (uint32_t)rnd(qlen - lead < 12 ? qlen - lead + 1 : 12);
            if (exact) offset = 0;
            if (lead) { cigar.push_back(lead << 3 | OP_CLIPPED); seen.lead_clip = true; }
            uint32_t left = qlen - lead - trail, qpos = lead, npos = 0;       // npos: node positions taken so far
            const uint32_t mean_run = q % 7 == 0 ? 4 : 12;
            uint32_t last_op = 7;
            bool ins_esc = false, mis_esc = false;
            if (qlen - lead - trail == 0) seen.unmapped = true;
            while (left) {
                uint32_t op;
                do {
                    const int c = (int)rnd(exact ? 4 : 10);
                    op = c < 3 ? OP_MATCH : c == 3 ? OP_MISMATCH : c < 7 ? OP_MATCH : c == 7 ? OP_INSERTION : c == 8 ? OP_DELETION : OP_MISMATCH;
                } while (op == last_op || (op == OP_INSERTION && (last_op == OP_DELETION)) || (op == OP_DELETION && last_op == OP_INSERTION));
                uint32_t len = 1 + (uint32_t)rnd(op == OP_MATCH ? 2 * mean_run : op == OP_INSERTION && rnd(4) == 0 ? 2 * k : 3);
                if (op != OP_DELETION && len > left) len = left;
                if (op == OP_DELETION && (left == 0 || npos == 0)) continue;      // (none at either end)
                const uint32_t cur = offset + npos;
                if (op == OP_INSERTION) {
                    if (cur < k) {
                        if (npos == 0) seen.ins_front = true; else seen.ins_inside = true;
                        if (len > k - cur) seen.ins_split = true;
                    } else seen.ins_before_node = true;
                }
                if (op == OP_DELETION) seen.deletion = true;
                if (op == OP_INSERTION || op == OP_MISMATCH)
                    for (uint32_t i = 0; i < len; ++i)
                        if (jf_esc_width(jf_strand_byte(strand, qpos + i)) > 1) (op == OP_INSERTION ? ins_esc : mis_esc) = true;
                if (op != OP_INSERTION) npos += len;
                if (op != OP_DELETION) { left -= len; qpos += len; }
                cigar.push_back(len << 3 | op);
                last_op = op;
            }
            if (trail) { cigar.push_back(trail << 3 | OP_CLIPPED); seen.trail_clip = true; }
            if (ins_esc) seen.esc_insertion[orientation] = true;
            if (mis_esc) seen.esc_mismatch[orientation] = true;
            // the nodes the runs pay for: the first takes k - offset positions, every other one a position
            uint32_t n_nodes;
            if (npos == 0) { n_nodes = (uint32_t)rnd(2); offset = n_nodes ? offset : 0; }
            else if (npos <= k - offset) { n_nodes = 1; if (npos < k - offset) seen.ends_in_first = true; }
            else n_nodes = npos - (k - offset) + 1;
            uint32_t n_cigar = (uint32_t)cigar.size();
            if (qlen == 0 && rnd(2)) { n_cigar = 0; cigar.clear(); }
            if (n_cigar > 64) seen.many_runs = true;
            if (offset && n_nodes) seen.offset = true;
            if (score < 0) seen.neg_score = true;
            (orientation ? seen.rev : seen.fwd) = true;
            seen.n_nodes.insert(n_nodes);
            const uint32_t seq_len = (uint32_t)rnd(9) == 0 ? 0 : n_nodes ? n_nodes + k - 1 - offset : (uint32_t)rnd(30);
            if (seq_len == 0) seen.no_seq = true;
            if (a == 0) { r.score = score; r.offset = offset; r.n_nodes = n_nodes; r.n_cigar = n_cigar; r.seq_len = seq_len; r.orientation = orientation; }
            else for (uint32_t w : { (uint32_t)score, offset, n_nodes, n_cigar, seq_len, orientation }) stream.push_back(w);
            const size_t nodes_at = stream.size();
            for (uint32_t x = 0; x < n_nodes; ++x) stream.push_back(node_id());
            if (n_nodes > 1 && rnd(5) == 0) { stream[nodes_at + n_nodes - 1] = stream[nodes_at]; }
            if (n_nodes > 1 && stream[nodes_at + n_nodes - 1] == stream[nodes_at]) seen.circular = true;
            for (uint32_t w : cigar) stream.push_back(w);
            std::string spelled;
            for (uint32_t x = 0; x < seq_len; ++x) spelled += "ACGTN$"[rnd(6)];
            spelled.resize((seq_len + 3) / 4 * 4, '#');                   // (padding: must never be printed)
            for (size_t x = 0; x < spelled.size(); x += 4) { uint32_t w; memcpy(&w, spelled.data() + x, 4); stream.push_back(w); }
            if (labeled) {
                const uint32_t nl = (uint32_t)rnd(25) == 0 ? 64 + (uint32_t)rnd(80) : (uint32_t)rnd(5);
                stream.push_back(nl);
                for (uint32_t x = 0; x < nl; ++x) stream.push_back((uint32_t)rng());
            }
        }
    }
    NEED(seen.secondary); NEED(seen.fwd); NEED(seen.rev); NEED(seen.neg_score); NEED(seen.lead_clip); NEED(seen.trail_clip);
    NEED(seen.ins_front); NEED(seen.ins_inside); NEED(seen.ins_split); NEED(seen.ins_before_node); NEED(seen.deletion);
    NEED(seen.ends_in_first); NEED(seen.offset); NEED(seen.circular); NEED(seen.no_seq); NEED(seen.unmapped); NEED(seen.many_runs);
    NEED(seen.empty_query); NEED(seen.esc_mismatch[0]); NEED(seen.esc_mismatch[1]); NEED(seen.esc_insertion[0]); NEED(seen.esc_insertion[1]);
    NEED(seen.node_1_digit); NEED(seen.node_10_digits); NEED(seen.no_alignment); NEED(seen.capacity); NEED(seen.hdr_empty); NEED(seen.hdr_long);
    for (uint32_t want : exact_nodes) NEED(seen.n_nodes.count(want));
    NEED(*seen.n_nodes.rbegin() > 128);

    const uint64_t stream_words = stream.size();
    seqs.append(8, '!'); headers.append(8, '!');
    stream.push_back(0x23232323u);

    // the whole batch, then three slices whose texts must concatenate to it
    const char sentinel = (char)0xA5;                  // (no byte of JSON text: every byte >= 0x7F is escaped)
    const size_t guard = 256;
    struct Range { uint64_t first, n; };
    const Range ranges[] = { { 0, n }, { 0, 97 }, { 97, 64 }, { 161, n - 161 } };
    std::vector<char> whole, joined;
    std::vector<uint64_t> whole_begin, joined_len;
    std::vector<uint32_t> whole_cap;
    for (size_t ri = 0; ri < 4; ++ri) {
        const Range rg = ranges[ri];
        std::vector<uint64_t> line_len(rg.n + 1, 0), line_begin(rg.n + 1, 0);
        std::vector<uint32_t> cap_list(rg.n + 1, 0);
        unsigned long long cap_count = 0;
        JfBatch b;
        memset(&b, 0, sizeof(b));
        b.results = rec.data(); b.stream = stream.data(); b.seqs = seqs.data(); b.offsets = offsets.data();
        b.headers = headers.data() + hoff[rg.first]; b.header_from = hoff[rg.first]; b.header_offsets = hoff.data() + rg.first;
        b.line_len = line_len.data(); b.line_begin = line_begin.data();
        b.cap_list = cap_list.data(); b.cap_count = &cap_count;
        b.first = rg.first; b.n_queries = rg.n; b.k = k; b.labeled = labeled ? 1 : 0;
        for (uint64_t i = 0; i < rg.n; ++i) line_len[i] = jf_line<false>(b, i);                    // size pass
        for (uint64_t i = 0; i < rg.n; ++i) line_begin[i + 1] = line_begin[i] + line_len[i];       // the scan
        std::vector<char> text;
        for (int shift = 0; shift < 2; ++shift) {
            std::vector<char> buf(line_begin[rg.n] + 2 * guard + 8, sentinel);
            b.text = buf.data() + guard + shift;
            for (uint64_t i = 0; i < rg.n; ++i) {
                const uint64_t wrote = jf_line<true>(b, i);                                         // write pass
                if (wrote != line_len[i]) { printf("FAIL query %llu: size pass %llu, write pass %llu\n", (unsigned long long)(rg.first + i), (unsigned long long)line_len[i], (unsigned long long)wrote); return false; }
            }
            for (size_t x = 0; x < buf.size(); ++x) {
                const bool inside = buf.data() + x >= b.text && buf.data() + x < b.text + line_begin[rg.n];
                if (inside && buf[x] == sentinel) { printf("FAIL: byte %zu of the text of range %zu was not written\n", x - guard - shift, ri); return false; }
                if (!inside && buf[x] != sentinel) { printf("FAIL: a byte outside the text was written (range %zu, shift %d)\n", ri, shift); return false; }
            }
            std::vector<char> t(b.text, b.text + line_begin[rg.n]);
            if (shift && t != text) { printf("FAIL: the text depends on its alignment\n"); return false; }
            text.swap(t);
        }
        if (ri == 0) { whole = text; whole_begin = line_begin; whole_cap.assign(cap_list.begin(), cap_list.begin() + cap_count); }
        else {
            joined.insert(joined.end(), text.begin(), text.end());
            for (uint64_t i = 0; i < rg.n; ++i) joined_len.push_back(line_len[i]);
            for (unsigned long long c = 0; c < cap_count; ++c)
                if (cap_list[c] + rg.first != cap_query) { printf("FAIL: the capacity list of a slice names query %llu\n", (unsigned long long)(cap_list[c] + rg.first)); return false; }
        }
    }
    if (joined != whole) { printf("FAIL: the slices' texts do not concatenate to the whole batch's\n"); return false; }
    for (uint64_t q = 0; q < n; ++q)
        if (joined_len[q] != whole_begin[q + 1] - whole_begin[q]) { printf("FAIL: query %llu has another length in its slice\n", (unsigned long long)q); return false; }
    if (whole_cap.size() != 1 || whole_cap[0] != cap_query) { printf("FAIL: the capacity list\n"); return false; }

    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const uint64_t hdr[8] = { n, labeled ? 1u : 0u, stream_words, offsets[n], hoff[n], k, whole_begin[n], whole_cap.size() };
    fwrite(hdr, 8, 8, f);
    put(f, rec, n); put(f, stream, stream_words); put(f, offsets, n + 1);
    fwrite(seqs.data(), 1, offsets[n], f);
    put(f, hoff, n + 1);
    fwrite(headers.data(), 1, hoff[n], f);
    put(f, whole_begin, n + 1); put(f, whole, whole.size()); put(f, whole_cap, whole_cap.size());
    fclose(f);
    return true;
}

// ---- jf_identity against the C library -------------------------------------------------------------------------------------
static uint64_t n_exponent = 0, n_carry = 0, n_checked = 0;

static bool identity_one(uint32_t m, uint32_t len) {
    char want[48], got[48], probe[48];
    const double v = len ? (double)m / (double)len : 0.0;
    snprintf(want, sizeof(want), "%.17g", v);
    if (!strpbrk(want, ".eEn")) strcat(want, ".0");
    memset(got, 0, sizeof(got));
    const uint32_t counted = jf_identity<false>(nullptr, m, len), wrote = jf_identity<true>(got, m, len);
    if (counted != wrote || strlen(got) != wrote || strcmp(got, want) != 0) {
        printf("FAIL identity %u / %u: \"%s\" (%u counted, %u written), want \"%s\"\n", m, len, got, counted, wrote, want);
        return false;
    }
    ++n_checked;
    if (strchr(want, 'e')) ++n_exponent;
    // the 17th significant digit rounded up out of a 9: "%.16e" ends in 0 where the longer expansion has a 9 there
    snprintf(probe, sizeof(probe), "%.16e", v);
    snprintf(want, sizeof(want), "%.25e", v);
    if (v != 0 && probe[17] == '0' && want[17] == '9') ++n_carry;
    return true;
}

static int identity() {
    for (uint32_t len = 0; len <= 2048; ++len)
        for (uint32_t m = 0; m <= len; ++m)
            if (!identity_one(m, len)) return 1;
    for (uint32_t len : { 9999u, 10000u, 10001u, 16384u, 32703u, 32704u })
        for (uint32_t m = 0; m <= len; ++m)
            if (!identity_one(m, len)) return 1;
    std::mt19937_64 rng(20250104);
    for (int i = 0; i < 1000000; ++i) {
        const uint32_t len = 1 + (uint32_t)(rng() % 32704), m = (uint32_t)(rng() % (len + 1));
        if (!identity_one(m, len)) return 1;
    }
    if (!n_exponent) { printf("FAIL: no value in exponent form\n"); return 1; }
    if (!n_carry) { printf("FAIL: no value whose 17th digit rounds with a carry\n"); return 1; }
    printf("ok identity: %llu pairs, %llu in exponent form, %llu round with a carry\n", (unsigned long long)n_checked,
           (unsigned long long)n_exponent, (unsigned long long)n_carry);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    static_assert(sizeof(ReadResult) == 64, "record layout");
    if (std::string(argv[1]) == "identity") return identity();
    // the escapes against the rule, every byte value
    for (uint32_t c = 1; c < 256; ++c) {
        char buf[8] = { 0 }, want[8];
        const uint32_t wd = jf_esc_width((char)c);
        jf_esc_put(buf, (char)c, wd);
        if (c == '"' || c == '\\') snprintf(want, sizeof(want), "\\%c", (char)c);
        else if (c == 8 || c == 9 || c == 10 || c == 12 || c == 13) snprintf(want, sizeof(want), "\\%c", c == 8 ? 'b' : c == 9 ? 't' : c == 10 ? 'n' : c == 12 ? 'f' : 'r');
        else if (c < 0x20 || c >= 0x7F) snprintf(want, sizeof(want), "\\u%04X", c);
        else snprintf(want, sizeof(want), "%c", (char)c);
        if (strlen(want) != wd || strcmp(buf, want) != 0) { printf("FAIL escape of byte %u: \"%s\", want \"%s\"\n", c, buf, want); return 1; }
    }
    const std::string prefix = argv[1];
    if (!variant(prefix + ".plain.bin", 20250201, false, 21)) return 1;
    if (!variant(prefix + ".labeled.bin", 20250202, true, 12)) return 1;
    if (!variant(prefix + ".small_k.bin", 20250203, false, 5)) return 1;
    printf("ok 3 variants\n");
    return 0;
}
