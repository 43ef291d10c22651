// cloud_io.hip -- raw point-cloud text on the device: a delimited table of decimal numbers -> float64 [rows, cols].
// Replaces the pandas.read_csv calls of the reference's dataset preparations (dataset/s3dis/prepare_data_inst.py:65,84,
// dataset/stpls3d/prepare_data_inst_instance_stpls3d.py:39,77) and the vertex lines of an ASCII PLY; the general
// sibling of result_io.hip's sg_parse_decimal_lines, on the same pattern:
//   lines   newline flags -> exclusive scan = physical line of every line start; the newline that ends line
//           `skip_lines` gives the offset where the data begins
//   rows    a line start is a row when its first byte that is no blank (space, tab, '\r') is neither '\n' nor the
//           comment byte -> exclusive scan = row index; the row's offset and line go to [rows] arrays
//   parse   one row per lane: tokens of at most 64 bytes through decimal.h (correctly rounded, or declined),
//           8-byte stores into the row's value slots
// Loops: the scans run over [0, nbytes); a lane walks blanks and one line, every read guarded by i < nbytes; a token
// is parsed from at most 64 bytes.  Stores: row r < rows (and < the rows found), field < cols.
// Text reaches the lanes a byte per load (the scans coalesce them across the wave; a row lane walks its own line out
// of the cache).  That is left so: on a 32 MB room the kernels take 0.5 ms, as much as the copy of the text to the
// device, and the two together a third of the call, whose rest is host copies (profiles/cloud_io_bench.txt).
#include "common.h"
#include "decimal.h"
#include "scan.h"

namespace sg {

constexpr int kCloudBlock = 256;
static int cloud_grid(int64_t items) { return grid_for(items, kCloudBlock, 2048); }

// meta words (include/softgroup_hip.h)
constexpr int kMetaLines = 0, kMetaRows = 1, kMetaDataOff = 2, kMetaDeclined = 3, kMetaMalformed = 4, kMetaBadLine = 5,
              kMetaStatus = 6, kMetaWords = 8;

__device__ __forceinline__ bool cloud_blank(uint8_t c) { return c == ' ' || c == '\t' || c == '\r'; }

// i is the first byte of a line that holds a row
__device__ __forceinline__ bool cloud_row_start(const uint8_t *__restrict__ text, int64_t nbytes, int64_t i, int comment) {
  if (i < 0 || i >= nbytes || (i != 0 && text[i - 1] != '\n')) return false;
  int64_t j = i;
  while (j < nbytes && cloud_blank(text[j])) ++j;
  return j < nbytes && text[j] != '\n' && static_cast<int>(text[j]) != comment;
}

__global__ void table_init_kernel(int64_t nbytes, int64_t skip_lines, int64_t *__restrict__ meta) {
  for (int k = 0; k < kMetaWords; ++k) meta[k] = 0;
  meta[kMetaDataOff] = skip_lines == 0 ? 0 : nbytes;       // (fewer lines than skipped: no data)
  meta[kMetaBadLine] = INT64_MAX;
}

__global__ void table_finish_kernel(const uint8_t *__restrict__ text, int64_t nbytes, const int32_t *__restrict__ newlines,
                                    const int32_t *__restrict__ rows_seen, int64_t rows, int64_t *__restrict__ meta) {
  meta[kMetaLines] = *newlines + (text[nbytes - 1] != '\n');
  meta[kMetaRows] = *rows_seen;
  if (rows >= 0 && *rows_seen != rows) meta[kMetaStatus] = 1;
}

// row r of the table: text from off[r] to the end of its line
__global__ void __launch_bounds__(kCloudBlock) table_rows_kernel(const uint8_t *__restrict__ text, int64_t nbytes, int delimiter,
                                                                int cols, int64_t rows, const int32_t *__restrict__ rows_seen,
                                                                const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ row_line,
                                                                double *__restrict__ values, uint8_t *__restrict__ row_status,
                                                                int64_t *__restrict__ meta) {
  const int64_t seen = *rows_seen;
  const int64_t n = seen < rows ? seen : rows;
  for (int64_t r = blockIdx.x * static_cast<int64_t>(kCloudBlock) + threadIdx.x; r < n;
       r += static_cast<int64_t>(gridDim.x) * kCloudBlock) {
    int64_t i = off[r];
    double *vrow = values + r * cols;
    unsigned st = 0;
    int field = 0;
    if (i < 0 || i >= nbytes) st = 2;
    while (st < 2) {
      while (i < nbytes && cloud_blank(text[i])) ++i;
      const bool at_end = i >= nbytes || text[i] == '\n';
      if (delimiter < 0) {
        if (at_end) break;
      } else if (at_end || static_cast<int>(text[i]) == delimiter) {
        st |= 2;                                         // an empty field
        break;
      }
      const int64_t t0 = i;
      bool bad = false;
      while (i < nbytes) {
        const uint8_t c = text[i];
        if (c == '\n' || cloud_blank(c) || static_cast<int>(c) == delimiter) break;
        bad |= c < 0x21 || c > 0x7E;
        ++i;
      }
      if (bad || i - t0 > kDecimalMaxToken || field >= cols) {
        st |= 2;
        break;
      }
      double v;
      const int s = decimal_to_double(text + t0, static_cast<int>(i - t0), &v);
      if (s == kDecimalOk) {
        vrow[field] = v;                                 // (field < cols, r < rows)
      } else if (s == kDecimalDeclined) {
        st |= 1;
      } else {
        st |= 2;
        break;
      }
      ++field;
      if (delimiter >= 0) {
        while (i < nbytes && cloud_blank(text[i])) ++i;
        if (i >= nbytes || text[i] == '\n') break;
        if (static_cast<int>(text[i]) != delimiter) {    // a second token inside one field
          st |= 2;
          break;
        }
        ++i;
      }
    }
    if (st < 2 && field != cols) st |= 2;
    row_status[r] = static_cast<uint8_t>(st);
    if (st & 2) {
      atomicAdd(reinterpret_cast<unsigned long long *>(meta + kMetaMalformed), 1ULL);
      atomicMin(reinterpret_cast<unsigned long long *>(meta + kMetaBadLine), static_cast<unsigned long long>(row_line[r]));
    } else if (st & 1) {
      atomicAdd(reinterpret_cast<unsigned long long *>(meta + kMetaDeclined), 1ULL);
    }
  }
}

struct TableScratch {
  int32_t *lineno, *off, *newlines, *rows_seen;
  void *sws;
  size_t sbytes;
};

static size_t table_half(int64_t nbytes) { return static_cast<size_t>(nbytes / 2 + 1); }

// the two scans; with row_line the rows' offsets and lines are recorded for r < rows
static int table_scan(const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment, int64_t rows, int32_t *row_line,
                      int64_t *meta, const TableScratch &t, hipStream_t stream) {
  int32_t *lineno = row_line ? t.lineno : nullptr;
  int rc = exclusive_scan(
      [text] __device__(int64_t i) { return text[i] == '\n' ? 1 : 0; },
      [text, nbytes, skip_lines, comment, lineno, meta] __device__(int64_t i, int line) {
        if (text[i] == '\n' && line + 1 == skip_lines) meta[kMetaDataOff] = i + 1;
        // a row's line holds a byte that is no blank and its '\n': row starts are two bytes apart at least
        if (lineno != nullptr && cloud_row_start(text, nbytes, i, comment)) lineno[i >> 1] = line;
      },
      nbytes, t.newlines, t.sws, t.sbytes, stream);
  if (rc != SG_OK) return rc;
  int32_t *off = t.off;
  const int64_t cap = static_cast<int64_t>(table_half(nbytes));
  return exclusive_scan(
      [text, nbytes, comment, meta] __device__(int64_t i) {
        return i >= meta[kMetaDataOff] && cloud_row_start(text, nbytes, i, comment) ? 1 : 0;
      },
      [text, nbytes, comment, meta, lineno, off, row_line, rows, cap] __device__(int64_t i, int r) {
        if (lineno == nullptr || r >= rows || r >= cap) return;
        if (i >= meta[kMetaDataOff] && cloud_row_start(text, nbytes, i, comment)) {
          off[r] = static_cast<int32_t>(i);
          row_line[r] = lineno[i >> 1] + 1;
        }
      },
      nbytes, t.rows_seen, t.sws, t.sbytes, stream);
}

static bool table_scratch(void *ws, size_t ws_bytes, int64_t nbytes, TableScratch *t) {
  Workspace a(ws, ws_bytes);
  t->lineno = a.take<int32_t>(table_half(nbytes));
  t->off = a.take<int32_t>(table_half(nbytes));
  t->sbytes = scan_workspace_bytes(nbytes > 0 ? nbytes : 1);
  t->sws = a.take<char>(t->sbytes);
  t->newlines = a.take<int32_t>(64);
  t->rows_seen = a.take<int32_t>(64);
  return t->rows_seen != nullptr;
}

static int table_args(const char *who, const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment,
                      const int64_t *meta) {
  SG_REQUIRE(nbytes >= 0 && nbytes < (1LL << 31) && skip_lines >= 0 && meta != nullptr && (nbytes == 0 || text != nullptr),
             "%s: bad arguments (%lld bytes, %lld lines skipped)", who, static_cast<long long>(nbytes),
             static_cast<long long>(skip_lines));
  SG_REQUIRE(comment < 0 || (comment > 0x20 && comment < 0x7F), "%s: comment byte %d: none (< 0) or printable ASCII", who,
             comment);
  return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_text_table_workspace_bytes(int64_t nbytes) {
  const int64_t m = nbytes > 0 ? nbytes : 1;
  return 2 * align_up(table_half(m) * 4) + align_up(scan_workspace_bytes(m)) + 2 * 256;
}

int sg_text_table_count(const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment, int64_t *meta, void *ws,
                        size_t ws_bytes, sg_stream_t stream_) {
  const int rc0 = table_args("sg_text_table_count", text, nbytes, skip_lines, comment, meta);
  if (rc0 != SG_OK) return rc0;
  TableScratch t;
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_text_table_workspace_bytes(nbytes) && table_scratch(ws, ws_bytes, nbytes, &t),
             "sg_text_table_count: workspace too small");
  hipStream_t stream = as_stream(stream_);
  table_init_kernel<<<1, 1, 0, stream>>>(nbytes, skip_lines, meta);
  if (nbytes == 0) return check_launch("sg_text_table_count");
  const int rc = table_scan(text, nbytes, skip_lines, comment, 0, nullptr, meta, t, stream);
  if (rc != SG_OK) return rc;
  table_finish_kernel<<<1, 1, 0, stream>>>(text, nbytes, t.newlines, t.rows_seen, -1, meta);
  return check_launch("sg_text_table_count");
}

int sg_text_table_parse(const uint8_t *text, int64_t nbytes, int64_t skip_lines, int comment, int delimiter, int cols,
                        int64_t rows, double *values, uint8_t *row_status, int32_t *row_line, int64_t *meta, void *ws,
                        size_t ws_bytes, sg_stream_t stream_) {
  const int rc0 = table_args("sg_text_table_parse", text, nbytes, skip_lines, comment, meta);
  if (rc0 != SG_OK) return rc0;
  SG_REQUIRE(cols >= 1 && cols <= 64 && rows >= 0 && (rows == 0 || (values && row_status && row_line)),
             "sg_text_table_parse: bad arguments (%d columns of 1..64, %lld rows)", cols, static_cast<long long>(rows));
  SG_REQUIRE(delimiter < 0 || (delimiter > 0x20 && delimiter < 0x7F),
             "sg_text_table_parse: delimiter byte %d: blanks (< 0) or printable ASCII", delimiter);
  TableScratch t;
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_text_table_workspace_bytes(nbytes) && table_scratch(ws, ws_bytes, nbytes, &t),
             "sg_text_table_parse: workspace too small");
  hipStream_t stream = as_stream(stream_);
  table_init_kernel<<<1, 1, 0, stream>>>(nbytes, skip_lines, meta);
  if (nbytes == 0) return check_launch("sg_text_table_parse");
  // (without rows there is nothing to record, but the rows found are still counted against `rows`)
  const int rc = table_scan(text, nbytes, skip_lines, comment, rows, rows ? row_line : nullptr, meta, t, stream);
  if (rc != SG_OK) return rc;
  table_finish_kernel<<<1, 1, 0, stream>>>(text, nbytes, t.newlines, t.rows_seen, rows, meta);
  if (rows)
    table_rows_kernel<<<cloud_grid(rows), kCloudBlock, 0, stream>>>(text, nbytes, delimiter, cols, rows, t.rows_seen, t.off,
                                                                   row_line, values, row_status, meta);
  return check_launch("sg_text_table_parse");
}

}  // extern "C"
