// col_plan.hpp — the host half of mgx_annotation_load_columns_device: the walk over a `.column.annodbg` image that parse_columns
// (boss_files.hpp) makes, with the Cursor, RawVec, skip and plan functions of boss_files.hpp / dbg_plan.hpp, without decoding a
// payload (plan_columns); the layout of a batch of bit vectors in the arena with its descriptor tables (BvBatch) for the kernel
// bodies of bv_decode.hpp; and one load's columns as such a batch (ColBatch) for those of col_decode.hpp.  Host code; used by mgx_colload.hip and by tests/emu/col_decode_check.cpp, which run the same ColBatch.
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

// A batch of bit vectors for the shared stage of bv_decode.hpp: the descriptor and prefix tables, and the vectors' places in the
// arena.  Vectors are added in label order; place() then lays the payloads out from `base` on — sections bt | btnr | low | high |
// plain bits, each in the order of adding, each closed by two zero words —, copies them into the stage, and gives every rrr
// vector and every sd vector that wants one a bit map from `tail` on (a stat vector's payload is its map).
struct BvBatch {
    std::vector<BvRrr> rrr;
    std::vector<CdSd> sd;
    std::vector<BvMap> map;
    std::vector<uint64_t> rbprefix{ 0 }, hprefix{ 0 }, bmprefix{ 0 };      // rrr.size() + 1, sd.size() + 1, map.size() + 1
    uint64_t payload_words = 10, tail_words = 0;
    uint32_t sd_maps = 0;                         // the sd vectors that have a bit map
    uint64_t rb_stride = 0, bm_stride = 0;        // the blocks of every rrr vector / the words of every bit map, 0: they differ (bv_find)
    std::vector<const RrrPlan *> rrr_src;         // (host only: the payloads, in images that outlive place())
    std::vector<const SdPlan *> sd_src;
    std::vector<const RawVec *> map_src;          // a stat vector's bits; nullptr: a map of the tail
    uint64_t rrr_blocks() const { return rbprefix.back(); }
    uint64_t high_words() const { return hprefix.back(); }
    uint64_t bm_words() const { return bmprefix.back(); }

    // a vector of `bits` bits for `label`; sd_map: an sd vector gets a bit map (rrr and stat vectors always have one)
    void add(const ColumnPlan &p, uint64_t bits, uint32_t label, bool sd_map) {
        const uint64_t words = (bits + 63) / 64;
        uint32_t kind = CD_KIND_STAT;
        if (p.code == CODE_SD) {
            kind = p.sd.inverted ? CD_KIND_SD_INVERTED : CD_KIND_SD;
            CdSd d{};
            d.high_bits = p.sd.high.bits; d.low_n = p.sd.low.size(); d.ones = p.sd.ones; d.wl = p.sd.wl; d.inverted = p.sd.inverted; d.label = label;
            d.map = sd_map ? (uint32_t)map.size() : BV_NO_MAP;
            sd.push_back(d);
            sd_src.push_back(&p.sd);
            hprefix.push_back(hprefix.back() + p.sd.high.words());
            payload_words += p.sd.low.words() + p.sd.high.words();
            sd_maps += sd_map;
            if (!sd_map) return;
        } else if (p.code == CODE_RRR) {
            kind = CD_KIND_RRR;
            BvRrr d{};
            d.btnr_bits = p.rrr.btnr.bits; d.bits = bits; d.label = label; d.map = (uint32_t)map.size();
            rb_stride = rrr.empty() || rb_stride == p.rrr.n_blocks ? p.rrr.n_blocks : 0;
            rrr.push_back(d);
            rrr_src.push_back(&p.rrr);
            rbprefix.push_back(rbprefix.back() + p.rrr.n_blocks);
            payload_words += p.rrr.bt.words() + p.rrr.btnr.words();
        } else payload_words += p.stat.v.words();
        bm_stride = map.empty() || bm_stride == words ? words : 0;
        map.push_back(BvMap{ 0, bits, p.code == CODE_STAT ? p.stat.ones : 0, kind, label });
        map_src.push_back(p.code == CODE_STAT ? &p.stat.v : nullptr);
        bmprefix.push_back(bmprefix.back() + words);
        if (p.code != CODE_STAT) tail_words += words;
    }
    // stage[base .. base + payload_words): zero before
    void place(uint64_t base, uint64_t tail, uint64_t *stage) {
        uint64_t at = base;
        auto put = [&](const RawVec &v, uint64_t &begin) {
            begin = at;
            if (v.words()) memcpy(stage + at, v.src, v.words() * 8);
            at += v.words();
        };
        for (size_t i = 0; i < rrr.size(); ++i) put(rrr_src[i]->bt, rrr[i].bt_begin);
        at += 2;
        for (size_t i = 0; i < rrr.size(); ++i) put(rrr_src[i]->btnr, rrr[i].btnr_begin);
        at += 2;
        for (size_t i = 0; i < sd.size(); ++i) put(sd_src[i]->low, sd[i].low_begin);
        at += 2;
        for (size_t i = 0; i < sd.size(); ++i) put(sd_src[i]->high, sd[i].high_begin);
        at += 2;
        for (size_t m = 0; m < map.size(); ++m) if (map_src[m]) put(*map_src[m], map[m].src_begin);
        at = tail;
        for (size_t m = 0; m < map.size(); ++m) if (!map_src[m]) { map[m].src_begin = at; at += bmprefix[m + 1] - bmprefix[m]; }
        for (BvRrr &d : rrr) d.bm_begin = map[d.map].src_begin;
        for (CdSd &d : sd) if (d.map != BV_NO_MAP) d.bm_begin = map[d.map].src_begin;
    }
};

// The buffers and tables of one load (all columns of all files, side by side in argument order; every file the same n_rows).
// arena: `upload_words` words copied from the host (stage) followed by the bit maps, which the device clears.
struct ColBatch {
    uint64_t n_rows = 0;
    std::vector<std::string> labels;
    BvBatch v;                                    // the columns, n_rows bits each; a plain sd column has no bit map
    std::vector<CdLabel> lab;
    std::vector<uint32_t> file_first;             // the first label of every file
    std::vector<uint64_t> stage;                  // the uploaded part of the arena
    uint64_t upload_words = 0, arena_words = 0;
    uint64_t extra_begin = 0;                     // the first of the `extra_upload` words of build()
    bool kinds[4] = { false, false, false, false };

    // plans[f] over images that outlive the call.  n_rows > 0 (an empty matrix has nothing to decode).
    // extra_upload: words kept free (zero) at the end of the uploaded part for payloads of the caller's (coord_plan.hpp)
    void build(const std::vector<ColumnsPlan> &plans, uint64_t extra_upload = 0) {
        n_rows = plans[0].n_rows;
        for (const ColumnsPlan &p : plans) {
            file_first.push_back((uint32_t)labels.size());
            labels.insert(labels.end(), p.labels.begin(), p.labels.end());
            for (const ColumnPlan &c : p.cols) {
                CdLabel l{ CD_KIND_SD, 0, 0, 0 };
                if (c.code == CODE_SD) { l.kind = c.sd.inverted ? CD_KIND_SD_INVERTED : CD_KIND_SD; l.sd = (uint32_t)v.sd.size(); }
                else l.kind = c.code == CODE_STAT ? CD_KIND_STAT : CD_KIND_RRR;
                if (l.kind != CD_KIND_SD) l.bm = (uint32_t)v.map.size();
                kinds[l.kind] = true;
                v.add(c, n_rows, (uint32_t)lab.size(), c.sd.inverted);
                lab.push_back(l);
            }
        }
        extra_begin = v.payload_words;
        upload_words = extra_begin + extra_upload;
        arena_words = upload_words + v.tail_words;
        stage.assign(upload_words, 0);
        v.place(0, upload_words, stage.data());
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
