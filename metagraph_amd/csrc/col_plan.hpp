// col_plan.hpp — the host half of mgx_annotation_load_columns_device: the walk over a `.column.annodbg` image that parse_columns
// (boss_files.hpp) makes, with the Cursor, RawVec, skip and plan functions of boss_files.hpp / dbg_plan.hpp, without decoding a
// payload (plan_columns); and the layout of one load's device buffers and descriptor tables (ColBatch) for the kernel bodies of
// col_decode.hpp.  Host code; used by mgx_colload.hip and by tests/emu/col_decode_check.cpp, which run the same ColBatch.
//
// A plan only ever answers "decode this on the device" or "ask the host reader": whenever it throws (a ParseError / Unsupported of
// the shared functions, or NeedsHost for the checks that parse_columns makes after it has decoded a payload), and whenever the
// device's error record is set, the caller runs parse_columns on the same image and returns ITS code and message — a damaged file
// gets the host reader's answer by construction, including which of two faults it names.
#pragma once
#include <algorithm>
#include <set>

#include "col_decode.hpp"
#include "dbg_plan.hpp"

namespace mgx { namespace files {

struct NeedsHost : std::runtime_error { using std::runtime_error::runtime_error; };

struct ColumnPlan { uint64_t code = CODE_SD; SdPlan sd; StatPlan stat; RrrPlan rrr; };
struct ColumnsPlan {
    uint64_t n_rows = 0;
    bool coded = true;                           // every column begins with a representation code (false: the bare bit_vector_sd
                                                 // columns of a `.column_coord.annodbg`, coord_plan.hpp)
    std::vector<std::string> labels;
    std::vector<ColumnPlan> cols;
};

inline ColumnsPlan plan_columns(const uint8_t *data, size_t n) {
    Cursor c(data, n);
    ColumnsPlan p;
    p.n_rows = c.be("num_rows");
    if (p.n_rows >= (1ull << 40)) throw ParseError("more rows than the device matrix addresses (2^40)");
    read_label_encoder(c, data, p.labels);
    p.cols.resize(p.labels.size());
    for (ColumnPlan &col : p.cols) {
        col.code = c.be("column");
        if (col.code == CODE_SD) {
            SdPlan &s = col.sd;
            s = plan_sd_vector(c, data, "column", p.n_rows);
            s.inverted = c.u8("column") != 0;
            // read_sd_vector's comparison of the select supports with popcount(high) = m: the device compares m with `ones`
            // (CD_SD_SELECT), so the other two terms can be taken with `ones` in m's place
            if (s.ones > s.high.bits || s.zeros != s.high.bits - s.ones || s.low.size() < s.ones) throw NeedsHost("column: select supports");
            // the guard of parse_columns on one inverted column; the one on the total: ColBatch::col_begin_from, after the counts
            if (s.inverted && s.size > (1ull << 33)) throw NeedsHost("column: inverted column of more than 2^33 rows");
        } else if (col.code == CODE_STAT) {
            col.stat = plan_bit_vector_stat(c, data, "column");
            if (col.stat.v.bits != p.n_rows) throw NeedsHost("inconsistent column size");
        } else if (col.code == CODE_RRR) {
            col.rrr = plan_rrr63(c, data, "column");
            if (col.rrr.bits != p.n_rows) throw NeedsHost("inconsistent column size");
        } else if (col.code == CODE_IL4096) throw Unsupported("column: bit_vector_il<4096> is not read");
        else throw ParseError("column: unknown bit vector representation " + std::to_string(col.code));
    }
    if (c.left()) throw ParseError("bytes left after the last column");
    return p;
}

// The buffers and tables of one load (all columns of all files, side by side in argument order; every file the same n_rows).
// arena: `upload_words` words copied from the host (stage) followed by the bit maps, which the device clears.
struct ColBatch {
    uint64_t n_rows = 0, W = 0, n_blocks = 0;    // W = ceil(n_rows / 64); n_blocks = ceil(n_rows / 63)
    std::vector<std::string> labels;
    std::vector<CdRrr> rrr;
    std::vector<CdSd> sd;
    std::vector<CdBm> bm;
    std::vector<CdLabel> lab;
    std::vector<uint64_t> hprefix{ 0 };           // sd.size() + 1
    std::vector<uint32_t> file_first;             // the first label of every file
    std::vector<uint64_t> stage;                  // the uploaded part of the arena
    uint64_t upload_words = 0, arena_words = 0;
    uint64_t extra_begin = 0;                     // the first of the `extra_upload` words of build()
    bool kinds[4] = { false, false, false, false };
    uint64_t high_words() const { return hprefix.back(); }
    uint64_t bm_words() const { return (uint64_t)bm.size() * W; }
    uint64_t rrr_blocks() const { return (uint64_t)rrr.size() * n_blocks; }

    // plans[f] over images that outlive the call.  n_rows > 0 (an empty matrix has nothing to decode).
    // extra_upload: words kept free (zero) at the end of the uploaded part for payloads of the caller's (coord_plan.hpp)
    void build(const std::vector<ColumnsPlan> &plans, uint64_t extra_upload = 0) {
        n_rows = plans[0].n_rows;
        W = (n_rows + 63) / 64;
        n_blocks = (n_rows + 62) / 63;
        std::vector<const ColumnPlan *> cols;
        for (const ColumnsPlan &p : plans) {
            file_first.push_back((uint32_t)labels.size());
            labels.insert(labels.end(), p.labels.begin(), p.labels.end());
            for (const ColumnPlan &c : p.cols) cols.push_back(&c);
        }
        lab.resize(cols.size());
        for (uint32_t j = 0; j < cols.size(); ++j) {
            const ColumnPlan &c = *cols[j];
            CdLabel &l = lab[j];
            l = CdLabel{ CD_KIND_SD, 0, 0, 0 };
            if (c.code == CODE_SD) {
                l.kind = c.sd.inverted ? CD_KIND_SD_INVERTED : CD_KIND_SD;
                l.sd = (uint32_t)sd.size();
                CdSd d{};
                d.high_bits = c.sd.high.bits; d.low_n = c.sd.low.size(); d.ones = c.sd.ones; d.wl = c.sd.wl; d.inverted = c.sd.inverted; d.label = j;
                sd.push_back(d);
                hprefix.push_back(hprefix.back() + c.sd.high.words());
            } else l.kind = c.code == CODE_STAT ? CD_KIND_STAT : CD_KIND_RRR;
            kinds[l.kind] = true;
            if (l.kind != CD_KIND_SD) {
                l.bm = (uint32_t)bm.size();
                bm.push_back(CdBm{ 0, c.code == CODE_STAT ? c.stat.ones : 0, l.kind, j });
            }
            if (c.code == CODE_RRR) {
                CdRrr d{};
                d.btnr_bits = c.rrr.btnr.bits; d.label = j;
                rrr.push_back(d);
            }
        }
        // sections of the uploaded part: bt | btnr | low | high | plain bits, each closed by two zero words
        uint64_t at = 0;
        auto section = [&](auto &&span_of, auto &&note) {
            for (uint32_t j = 0; j < cols.size(); ++j) {
                const RawVec *v = span_of(*cols[j]);
                if (!v) continue;
                note(j, at);
                at += v->words();
            }
            at += 2;
        };
        uint32_t x = 0;
        section([](const ColumnPlan &c) { return c.code == CODE_RRR ? &c.rrr.bt : nullptr; }, [&](uint32_t, uint64_t o) { rrr[x++].bt_begin = o; });
        x = 0;
        section([](const ColumnPlan &c) { return c.code == CODE_RRR ? &c.rrr.btnr : nullptr; }, [&](uint32_t, uint64_t o) { rrr[x++].btnr_begin = o; });
        section([](const ColumnPlan &c) { return c.code == CODE_SD ? &c.sd.low : nullptr; }, [&](uint32_t j, uint64_t o) { sd[lab[j].sd].low_begin = o; });
        section([](const ColumnPlan &c) { return c.code == CODE_SD ? &c.sd.high : nullptr; }, [&](uint32_t j, uint64_t o) { sd[lab[j].sd].high_begin = o; });
        section([](const ColumnPlan &c) { return c.code == CODE_STAT ? &c.stat.v : nullptr; }, [&](uint32_t j, uint64_t o) { bm[lab[j].bm].src_begin = o; });
        extra_begin = at;
        at += extra_upload;
        upload_words = at;
        stage.assign(upload_words, 0);
        auto copy = [&](const RawVec &v, uint64_t o) { if (v.words()) memcpy(stage.data() + o, v.src, v.words() * 8); };
        x = 0;
        for (uint32_t j = 0; j < cols.size(); ++j) {
            const ColumnPlan &c = *cols[j];
            if (c.code == CODE_RRR) { copy(c.rrr.bt, rrr[x].bt_begin); copy(c.rrr.btnr, rrr[x].btnr_begin); ++x; }
            else if (c.code == CODE_SD) { copy(c.sd.low, sd[lab[j].sd].low_begin); copy(c.sd.high, sd[lab[j].sd].high_begin); }
            else copy(c.stat.v, bm[lab[j].bm].src_begin);
        }
        // the bit maps behind them
        x = 0;
        for (uint32_t j = 0; j < cols.size(); ++j) {
            if (lab[j].kind == CD_KIND_RRR) { rrr[x].bm_begin = at; bm[lab[j].bm].src_begin = at; at += W; ++x; }
            else if (lab[j].kind == CD_KIND_SD_INVERTED) { sd[lab[j].sd].bm_begin = at; bm[lab[j].bm].src_begin = at; at += W; }
        }
        arena_words = at;
    }

    // col_begin from the per-column counts; false: parse_columns' guard on the total of expanded rows (an inverted column reached
    // with more than 2^33 rows of its file in all) — the host reader is asked
    bool col_begin_from(const std::vector<uint64_t> &counts, std::vector<uint64_t> &col_begin) const {
        col_begin.assign(1, 0);
        uint64_t file_base = 0;
        for (uint32_t j = 0, f = 0; j < lab.size(); ++j) {
            for (; f < file_first.size() && file_first[f] <= j; ++f) file_base = col_begin.back();
            if (lab[j].kind == CD_KIND_SD_INVERTED && col_begin.back() - file_base + n_rows > (1ull << 33)) return false;
            if (counts[j] > n_rows) return false;
            col_begin.push_back(col_begin.back() + counts[j]);
        }
        return true;
    }
};

// plans of several images into one batch; throws what mgx_column_file_read throws for files that do not go together
inline void check_merge(const std::vector<ColumnsPlan> &plans) {
    std::set<std::string> seen;
    for (size_t f = 0; f < plans.size(); ++f) {
        if (f && plans[f].n_rows != plans[0].n_rows) throw NeedsHost("row counts differ");
        for (const std::string &l : plans[f].labels) if (!seen.insert(l).second) throw NeedsHost("label occurs in two files");
    }
}

}}  // namespace mgx::files
