// column_file.hpp — the object behind mgx_column_file (include/mgx.h, "files"), shared by the units that make one:
// mgx_files.hip (mgx_column_file_read) and mgx_colload.hip (the names_out of mgx_annotation_load_columns_device).
#pragma once
#include "boss_files.hpp"

namespace mgx { namespace files {
inline bool path_ends_with(const std::string &p, const std::string &ext) { return p.size() >= ext.size() && !p.compare(p.size() - ext.size(), ext.size(), ext); }
// form (b) of a coordinate annotation (boss_files.hpp: parse_column_coord); any other path is a column file of form (a)
inline bool is_column_coord_path(const std::string &p) { return path_ends_with(p, ".column_coord.annodbg"); }
// X.column.annodbg -> X.column.annodbg.coords (load_coords, annotation_converters.cpp:1711-1712: remove_suffix(file, kExtension) +
// kCoordExtension)
inline std::string coord_side_path(const std::string &p) {
    static const std::string ext = ".column.annodbg";
    return (path_ends_with(p, ext) ? p.substr(0, p.size() - ext.size()) : p) + ".column.annodbg.coords";
}
}}  // namespace mgx::files

struct mgx_column_file {
    mgx::files::ColumnFile f;
    bool rows_on_device = false;     // names_out of mgx_annotation_load_columns_device: n_rows, labels and col_begin only
};
