// coord_plan.hpp — the host half of mgx_annotation_load_coord_columns_device: the walk over the tuple section that read_tuples
// (boss_files.hpp) makes, and over a `.column_coord.annodbg` image as parse_column_coord makes it, without decoding a payload; and
// the layout of the coordinate part of one load's arena and its tables (CoordBatch: the delimiter vectors as a BvBatch of
// col_plan.hpp, and the values) for the cq_* bodies of coord_decode.hpp.  Host code; used by mgx_colload.hip and tests/emu/coord_decode_check.cpp, which run the same batch.
// As in col_plan.hpp a plan answers "decode this on the device" or "ask the host reader" (any exception), nothing else.
#pragma once
#include "col_plan.hpp"
#include "coord_decode.hpp"

namespace mgx { namespace files {

// one column of the tuple section: the delimiters (a bit_vector_smart: code + vector) and the values (sdsl::int_vector<>)
struct TuplePlan : ColumnPlan {
    RawVec values;
    uint64_t bits() const { return code == CODE_SD ? sd.size : code == CODE_STAT ? stat.v.bits : rrr.bits; }
};

// the tuple section of n_cols columns; the checks that need the columns' set rows or a payload are the kernels' and
// CoordBatch::lengths_fit's
inline std::vector<TuplePlan> plan_tuples(Cursor &c, const uint8_t *data, size_t n_cols, uint64_t n_rows) {
    std::vector<TuplePlan> out(n_cols);
    for (TuplePlan &t : out) {
        t.code = c.be("delimiters");
        if (t.code == CODE_SD) {
            {   // read_tuples bounds the length field by the file and the column's set rows (at most n_rows) before it builds the vector
                Cursor peek = c;
                if (peek.le("delimiters") > (uint64_t)c.left() * 8 + n_rows + 1) throw NeedsHost("delimiters: size field");
            }
            Cursor peek = c;
            t.sd = plan_sd_vector(c, data, "delimiters", peek.le("delimiters"));
            t.sd.inverted = c.u8("delimiters") != 0;
            if (t.sd.ones > t.sd.high.bits || t.sd.zeros != t.sd.high.bits - t.sd.ones || t.sd.low.size() < t.sd.ones) throw NeedsHost("delimiters: select supports");
        } else if (t.code == CODE_STAT) t.stat = plan_bit_vector_stat(c, data, "delimiters");
        else if (t.code == CODE_RRR) t.rrr = plan_rrr63(c, data, "delimiters");
        else if (t.code == CODE_IL4096) throw Unsupported("delimiters: bit_vector_il<4096> is not read");
        else throw ParseError("delimiters: unknown bit vector representation " + std::to_string(t.code));
        t.values = raw_behind(c, data, read_int_vector(c, "values", false));
        if (!t.bits()) throw NeedsHost("delimiters: no bits");
    }
    if (c.left()) throw ParseError("bytes left after the last column");
    return out;
}

// Form (b), `.column_coord.annodbg`: the binary columns are bit_vector_sd WITHOUT a representation code (ColumnMajor::serialize,
// column_major.cpp:110-123) — the plan says so (coded = false) instead of reading a code that is not there — and there is no
// num_rows field: the first column's size is the row count, a column of another size is for the host reader to name.
inline ColumnsPlan plan_column_coord(const uint8_t *data, size_t n, std::vector<TuplePlan> &tuples) {
    Cursor c(data, n);
    ColumnsPlan p;
    p.coded = false;
    read_label_encoder(c, data, p.labels);
    if (c.be("number of columns") != p.labels.size()) throw NeedsHost("number of columns");
    p.cols.resize(p.labels.size());
    for (size_t j = 0; j < p.cols.size(); ++j) {
        if (!j) {
            Cursor peek = c;
            p.n_rows = peek.le("column");
            if (p.n_rows >= (1ull << 40)) throw NeedsHost("more rows than the device matrix addresses (2^40)");
        }
        ColumnPlan &col = p.cols[j];
        col.code = CODE_SD;
        SdPlan &s = col.sd;
        s = plan_sd_vector(c, data, "column", p.n_rows);
        s.inverted = c.u8("column") != 0;
        if (s.ones > s.high.bits || s.zeros != s.high.bits - s.ones || s.low.size() < s.ones) throw NeedsHost("column: select supports");
        if (s.inverted && s.size > (1ull << 33)) throw NeedsHost("column: inverted column of more than 2^33 rows");
    }
    tuples = plan_tuples(c, data, p.cols.size(), p.n_rows);
    return p;
}

// The coordinate part of one load: all columns of all files in argument order, like ColBatch.  Its payloads lie in the arena's
// uploaded part at [base, base + upload_words) — the sections of the delimiter vectors (BvBatch: every one gets a bit map), then
// the values, closed by two zero words —, the bit maps of the sd and rrr delimiter vectors behind everything else at
// [tail, tail + v.tail_words).
struct CoordBatch {
    BvBatch v;                                    // the delimiter vectors; map j is column j's
    std::vector<CqCol> col;
    std::vector<uint64_t> vprefix{ 0 };
    uint64_t upload_words = 0;
    uint64_t n_values() const { return vprefix.back(); }

    void layout(const std::vector<const TuplePlan *> &t) {
        upload_words = 2;
        for (uint32_t j = 0; j < t.size(); ++j) {
            col.push_back(CqCol{ 0, t[j]->values.width, (uint32_t)v.sd.size() });
            v.add(*t[j], t[j]->bits(), j, true);
            vprefix.push_back(vprefix.back() + t[j]->values.size());
            upload_words += t[j]->values.words();
        }
        upload_words += v.payload_words;
    }
    // the payloads into stage[base .. base + upload_words) (zero before)
    void place(const std::vector<const TuplePlan *> &t, uint64_t base, uint64_t tail, uint64_t *stage) {
        v.place(base, tail, stage);
        uint64_t at = base + v.payload_words;
        for (uint32_t j = 0; j < t.size(); ++j) {
            const RawVec &x = t[j]->values;
            col[j].val_begin = at;
            if (x.words()) memcpy(stage + at, x.src, x.words() * 8);
            at += x.words();
        }
    }
    // read_tuples' first condition, once the columns' set rows are counted: bits = values + set rows + 1
    bool lengths_fit(const std::vector<uint64_t> &col_begin) const {
        for (uint32_t j = 0; j < col.size(); ++j)
            if (v.map[j].bits != (vprefix[j + 1] - vprefix[j]) + (col_begin[j + 1] - col_begin[j]) + 1) return false;
        return true;
    }
};

}}  // namespace mgx::files
