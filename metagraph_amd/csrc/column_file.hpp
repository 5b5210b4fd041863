// column_file.hpp — the object behind mgx_column_file (include/mgx.h, "files"), shared by the units that make one:
// mgx_files.hip (mgx_column_file_read) and mgx_colload.hip (the names_out of mgx_annotation_load_columns_device).
#pragma once
#include "boss_files.hpp"

struct mgx_column_file {
    mgx::files::ColumnFile f;
    bool rows_on_device = false;     // names_out of mgx_annotation_load_columns_device: n_rows, labels and col_begin only
};
