// result_io.hip -- the text and label files of the test loop's --out directory, formatted and parsed on the
// device.  Replaces the per-file work of the reference's tools/test.py:40-107: save_single_instance decodes
// every run-length string to a dense vector and prints it with np.savetxt(fmt='%d') -- one '0' or '1' and a
// newline per point, 0.2 s of one core per 150 000-point mask -- save_gt_instance prints one decimal id per
// point the same way, save_panoptic_single sends every class through np.vectorize(dict.__getitem__).
//
// Everything here is a streaming kernel, bytes-bound; the mask text and the panoptic words go out as 16-byte
// stores, the decimal lines (variable width, a few bytes per point) as single bytes at their scanned offsets:
//   mask text     every lane owns 16 output bytes = 8 points of the instance-major text of `count` masks and
//                 stores them as one uint4; the masks come as runs (one binary search per lane, then a walk)
//                 or as bit rows (one word per 32 points).  Rows are length * 2 bytes long, so the lanes cut
//                 the FLAT text, not the rows: a lane whose 8 points straddle two masks seeks again.
//   decimal lines width of every value -> exclusive scan -> digits; optional ScanNet NYU remap in front.
//   panoptic      class through a table, (cls & 0xFFFF) | (id << 16), four words per lane.
//   readers       newline flags -> exclusive scan = line number of every line start -> one line per lane;
//                 mask text is fixed pitch (2 bytes per point): 64 bytes per lane -> 32 flags + one bit word.
// The readers accept exactly what the writers (and np.savetxt(fmt='%d')) emit and count everything else.
#include "common.h"
#include "scan.h"

namespace sg {

constexpr int kIoBlock = 256;
static int io_grid(int64_t items) { return grid_for(items, kIoBlock, 2048); }

// ---- mask sources: seek(instance, point) then test(point) for ascending points of that instance --------
struct RunSource {
  const int32_t *starts, *ends;
  const int64_t *bounds;
  int64_t n_runs;
  int64_t r, hi;
  int32_t cs, ce;
  __device__ __forceinline__ void load() {
    if (r < hi) cs = starts[r], ce = ends[r];
  }
  __device__ __forceinline__ void seek(int64_t inst, int64_t idx) {
    int64_t lo = bounds[inst];
    hi = bounds[inst + 1];
    lo = lo < 0 ? 0 : (lo > n_runs ? n_runs : lo);          // (a corrupt table must not leave the run arrays)
    hi = hi < lo ? lo : (hi > n_runs ? n_runs : hi);
    int64_t a = lo, b = hi;                                  // first run that ends behind idx
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (ends[m] > idx) b = m; else a = m + 1;
    }
    r = a;
    load();
  }
  __device__ __forceinline__ uint32_t test(int64_t idx) {
    while (r < hi && ce <= idx) {
      ++r;
      load();
    }
    return r < hi && cs <= idx ? 1u : 0u;
  }
};

struct BitSource {
  const uint32_t *bits;
  int64_t words;
  const uint32_t *row;
  uint32_t w;
  __device__ __forceinline__ void seek(int64_t inst, int64_t idx) {
    row = bits + inst * words;
    w = row[idx >> 5];
  }
  __device__ __forceinline__ uint32_t test(int64_t idx) {
    if ((idx & 31) == 0) w = row[idx >> 5];
    return (w >> (idx & 31)) & 1u;
  }
};

// text[2 p], text[2 p + 1] = '0' + bit, '\n' for the flat point p = instance * length + point
template <typename Src>
__global__ void __launch_bounds__(kIoBlock) mask_text_kernel(Src src0, int first, int64_t length, int64_t total_points,
                                                            uint8_t *__restrict__ text) {
  const int64_t chunks = (total_points + 7) / 8;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(kIoBlock) + threadIdx.x; g < chunks;
       g += static_cast<int64_t>(gridDim.x) * kIoBlock) {
    Src src = src0;
    const int64_t p = 8 * g;
    int64_t inst = p / length, idx = p - inst * length;
    src.seek(first + inst, idx);
    const int cnt = total_points - p >= 8 ? 8 : static_cast<int>(total_points - p);
    uint32_t q[4] = {0x0A300A30u, 0x0A300A30u, 0x0A300A30u, 0x0A300A30u};     // "0\n0\n", little endian
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < cnt) {
        q[j >> 1] |= src.test(idx) << ((j & 1) * 16);
        if (++idx == length && j + 1 < cnt) {
          ++inst;
          idx = 0;
          src.seek(first + inst, 0);
        }
      }
    }
    if (cnt == 8) {
      *reinterpret_cast<uint4 *>(text + 16 * g) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      for (int j = 0; j < 2 * cnt; ++j) text[16 * g + j] = static_cast<uint8_t>(q[j >> 2] >> ((j & 3) * 8));
    }
  }
}

// ---- decimal lines ---------------------------------------------------------------------------------------
__device__ __forceinline__ int io_digits32(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5
       : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}
__device__ __forceinline__ int io_digits64(uint64_t m) {
  if ((m >> 32) == 0) return io_digits32(static_cast<uint32_t>(m));
  int d = 10;
  uint64_t p = 10000000000ULL;
  while (d < 20 && m >= p) {
    ++d;
    p *= 10;       // (10^19 still fits; the loop ends before 10^20 would be needed)
  }
  return d;
}
__device__ __forceinline__ uint64_t io_magnitude(int64_t v) {
  return v < 0 ? 0ULL - static_cast<uint64_t>(v) : static_cast<uint64_t>(v);      // (INT64_MIN -> 2^63)
}
__device__ __forceinline__ int io_line_width(int64_t v) { return (v < 0) + io_digits64(io_magnitude(v)) + 1; }

// save_gt_instance's remap (tools/test.py:68-77) with numpy's floor division; *bad when nyu_id[sem - 1] is an
// IndexError in the reference.  sem == 0 (ignore) stays 0 without a table read.
__device__ __forceinline__ int64_t io_remap(int64_t v, const int32_t *__restrict__ table, int len, bool *bad) {
  if (table == nullptr) return v;
  int64_t sem = v / 1000, ins = v % 1000;
  if (ins < 0) {
    ins += 1000;
    sem -= 1;
  }
  if (sem == 0) return ins;
  int64_t k = sem - 1;
  if (k < 0) k += len;                     // (numpy's negative index)
  if (k < 0 || k >= len) {
    *bad = true;
    return 0;
  }
  return static_cast<int64_t>(table[k]) * 1000 + ins;
}

// meta[0] = bytes of text, meta[1] = values whose table index is out of range, meta[2] = lines that did not fit
__global__ void __launch_bounds__(kIoBlock) decimal_lines_kernel(const int64_t *__restrict__ values, int64_t n,
                                                                const int32_t *__restrict__ table, int table_len,
                                                                const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ total, int64_t capacity,
                                                                uint8_t *__restrict__ text, int64_t *__restrict__ meta) {
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[0] = *total;
  for (int64_t i = blockIdx.x * static_cast<int64_t>(kIoBlock) + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kIoBlock) {
    bool bad = false;
    const int64_t v = io_remap(values[i], table, table_len, &bad);
    if (bad) atomicAdd(reinterpret_cast<unsigned long long *>(meta + 1), 1ULL);
    uint64_t m = io_magnitude(v);
    const int d = io_digits64(m), neg = v < 0;
    const int64_t o = off[i];
    if (o + neg + d + 1 > capacity) {
      atomicAdd(reinterpret_cast<unsigned long long *>(meta + 2), 1ULL);
      continue;
    }
    uint8_t *p = text + o;
    if (neg) *p++ = '-';
    int k = d - 1;
    for (; (m >> 32) != 0; --k) {
      p[k] = static_cast<uint8_t>('0' + m % 10);
      m /= 10;
    }
    for (uint32_t s = static_cast<uint32_t>(m); k >= 0; --k) {
      p[k] = static_cast<uint8_t>('0' + s % 10u);
      s /= 10u;
    }
    p[d] = '\n';
  }
}

// ---- panoptic words (save_panoptic_single, tools/test.py:91-107) -----------------------------------------
constexpr int32_t kIoNoKey = INT32_MIN;      // table entry of a class the map lacks

// missing[0] += points without an entry; missing[1] = min over them of (index << 16 | class)
__global__ void __launch_bounds__(kIoBlock) panoptic_words_kernel(const uint32_t *__restrict__ words, int64_t n, bool vec,
                                                                 const int32_t *__restrict__ lut, int lut_len,
                                                                 uint32_t *__restrict__ out,
                                                                 unsigned long long *__restrict__ missing) {
  const int64_t quads = (n + 3) / 4;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(kIoBlock) + threadIdx.x; g < quads;
       g += static_cast<int64_t>(gridDim.x) * kIoBlock) {
    const int64_t i0 = 4 * g;
    const int cnt = n - i0 >= 4 ? 4 : static_cast<int>(n - i0);
    uint32_t w[4];
    if (cnt == 4 && vec) {
      const uint4 q = *reinterpret_cast<const uint4 *>(words + i0);
      w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) w[b] = b < cnt ? words[i0 + b] : 0u;
    }
    uint32_t r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int cls = static_cast<int>(w[b] & 0xFFFFu);
      const int32_t l = cls < lut_len ? lut[cls] : kIoNoKey;
      if (l == kIoNoKey && b < cnt) {
        atomicAdd(missing, 1ULL);
        atomicMin(missing + 1, (static_cast<unsigned long long>(i0 + b) << 16) | static_cast<unsigned>(cls));
      }
      r[b] = (static_cast<uint32_t>(l) & 0xFFFFu) | (w[b] & 0xFFFF0000u);
    }
    if (cnt == 4 && vec) {
      *reinterpret_cast<uint4 *>(out + i0) = make_uint4(r[0], r[1], r[2], r[3]);
    } else {
      for (int b = 0; b < cnt; ++b) out[i0 + b] = r[b];
    }
  }
}

// ---- readers ---------------------------------------------------------------------------------------------
// One line, from its first byte: optional '-', 1..19 digits, '\n' or the end of the text.  false: anything else
// (or a value outside int64).
__device__ __forceinline__ bool io_parse_line(const uint8_t *__restrict__ text, int64_t i, int64_t nbytes, int64_t *out) {
  const bool neg = text[i] == '-';
  if (neg) ++i;
  uint64_t m = 0;
  int d = 0;
  for (; i < nbytes; ++i, ++d) {
    const uint8_t c = text[i];
    if (c == '\n') break;
    if (c < '0' || c > '9' || d == 19) return false;
    m = m * 10 + (c - '0');            // (19 digits stay below 2^64)
  }
  if (d == 0 || m > (1ULL << 63) - (neg ? 0 : 1)) return false;
  *out = neg ? static_cast<int64_t>(0ULL - m) : static_cast<int64_t>(m);
  return true;
}

__global__ void parse_lines_finish_kernel(const uint8_t *__restrict__ text, int64_t nbytes,
                                          const int32_t *__restrict__ newlines, int64_t *__restrict__ meta) {
  meta[0] = *newlines + (text[nbytes - 1] != '\n');
}

// 64 bytes of text = 32 points per lane: flags[32] as two uint4, one bit word.  meta[0] = points, meta[1] += bad
// points.
__global__ void __launch_bounds__(kIoBlock) parse_mask_kernel(const uint8_t *__restrict__ text, int64_t nbytes,
                                                             int64_t n_points, uint8_t *__restrict__ flags,
                                                             uint32_t *__restrict__ bits, int64_t *__restrict__ meta) {
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[0] = n_points;
  const int64_t groups = (n_points + 31) / 32;
  for (int64_t g = blockIdx.x * static_cast<int64_t>(kIoBlock) + threadIdx.x; g < groups;
       g += static_cast<int64_t>(gridDim.x) * kIoBlock) {
    const int64_t b0 = 64 * g;
    uint32_t word = 0, bad = 0;
    if (b0 + 64 <= nbytes) {
      uint32_t f[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint4 q = *reinterpret_cast<const uint4 *>(text + b0 + 16 * c);
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // "b\nb\n": both flag bytes '0' | '1', both separators '\n'
          bad += ((u[k] & 0xFFFEFFFEu) != 0x0A300A30u);
          const uint32_t lo = u[k] & 1u, hi = (u[k] >> 16) & 1u;
          word |= (lo | (hi << 1)) << (8 * c + 2 * k);
          const uint32_t pair = lo | (hi << 8);          // flag bytes 8 c + 2 k and the next of this lane's 32
          if ((k & 1) == 0)
            f[2 * c + (k >> 1)] = pair;
          else
            f[2 * c + (k >> 1)] |= pair << 16;
        }
      }
      if (flags) {
        uint4 *o = reinterpret_cast<uint4 *>(flags + 32 * g);
        o[0] = make_uint4(f[0], f[1], f[2], f[3]);
        o[1] = make_uint4(f[4], f[5], f[6], f[7]);
      }
    } else {                                             // the last lane: byte by byte
      const int cnt = static_cast<int>(n_points - 32 * g);
      for (int j = 0; j < cnt; ++j) {
        const int64_t b = b0 + 2 * j;
        const uint8_t c = text[b];
        const bool sep = b + 1 < nbytes ? text[b + 1] == '\n' : true;     // (the final newline may be missing)
        bad += !((c == '0' || c == '1') && sep);
        word |= static_cast<uint32_t>(c & 1) << j;
        if (flags) flags[32 * g + j] = c & 1;
      }
    }
    if (bits) bits[g] = word;
    if (bad) atomicAdd(reinterpret_cast<unsigned long long *>(meta + 1), static_cast<unsigned long long>(bad));
  }
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace sg

using namespace sg;

extern "C" {

static int mask_text_args(const char *who, int n_inst, int64_t length, int first, int count, const uint8_t *text,
                          int64_t text_capacity) {
  SG_REQUIRE(n_inst >= 0 && length >= 0 && length < (1LL << 31), "%s: bad arguments (n_inst %d, length %lld)", who, n_inst,
             static_cast<long long>(length));
  SG_REQUIRE(first >= 0 && count >= 0 && static_cast<int64_t>(first) + count <= n_inst,
             "%s: instances [%d, %d + %d) outside [0, %d)", who, first, first, count, n_inst);
  SG_REQUIRE(count == 0 || length == 0 || (text != nullptr && aligned16(text)), "%s: text must be 16-byte aligned", who);
  SG_REQUIRE(text_capacity >= static_cast<int64_t>(count) * length * 2, "%s: text buffer %lld < %lld bytes", who,
             static_cast<long long>(text_capacity), static_cast<long long>(count) * length * 2);
  return SG_OK;
}

int sg_mask_text_runs(const int32_t *starts, const int32_t *ends, const int64_t *bounds, int64_t n_runs, int n_inst,
                      int64_t length, int first, int count, uint8_t *text, int64_t text_capacity, sg_stream_t stream) {
  const int rc = mask_text_args("sg_mask_text_runs", n_inst, length, first, count, text, text_capacity);
  if (rc != SG_OK) return rc;
  SG_REQUIRE(n_runs >= 0 && bounds != nullptr && (n_runs == 0 || (starts && ends)), "sg_mask_text_runs: bad arguments");
  const int64_t total = static_cast<int64_t>(count) * length;
  if (total == 0) return SG_OK;
  RunSource src{starts, ends, bounds, n_runs, 0, 0, 0, 0};
  mask_text_kernel<<<io_grid((total + 7) / 8), kIoBlock, 0, as_stream(stream)>>>(src, first, length, total, text);
  return check_launch("sg_mask_text_runs");
}

int sg_mask_text_bits(const uint32_t *bits, int n_inst, int64_t length, int first, int count, uint8_t *text,
                      int64_t text_capacity, sg_stream_t stream) {
  const int rc = mask_text_args("sg_mask_text_bits", n_inst, length, first, count, text, text_capacity);
  if (rc != SG_OK) return rc;
  const int64_t total = static_cast<int64_t>(count) * length;
  SG_REQUIRE(total == 0 || bits != nullptr, "sg_mask_text_bits: bad arguments");
  if (total == 0) return SG_OK;
  BitSource src{bits, (length + 31) / 32, nullptr, 0};
  mask_text_kernel<<<io_grid((total + 7) / 8), kIoBlock, 0, as_stream(stream)>>>(src, first, length, total, text);
  return check_launch("sg_mask_text_bits");
}

constexpr int64_t kIoMaxLines = (1LL << 31) / 21 - 1;     // 21 bytes per line at most: the offsets are int32

size_t sg_decimal_lines_workspace_bytes(int64_t n) {
  const int64_t m = n > 0 ? n : 1;
  return align_up(static_cast<size_t>(m) * 4) + align_up(scan_workspace_bytes(m)) + 512;
}

int sg_decimal_lines(const int64_t *values, int64_t n, const int32_t *nyu_table, int nyu_len, uint8_t *text,
                     int64_t text_capacity, int64_t *meta, void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && n <= kIoMaxLines && meta != nullptr && text_capacity >= 0 && (n == 0 || (values && text)) &&
                 (nyu_table == nullptr || nyu_len > 0),
             "sg_decimal_lines: bad arguments (n %lld)", static_cast<long long>(n));
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_decimal_lines_workspace_bytes(n), "sg_decimal_lines: workspace too small");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 3 * sizeof(int64_t), stream);
  if (n == 0) return check_launch("sg_decimal_lines");
  Workspace a(ws, ws_bytes);
  int32_t *off = a.take<int32_t>(n);
  const size_t sbytes = scan_workspace_bytes(n);
  void *sws = a.take<char>(sbytes);
  int32_t *total = a.take<int32_t>(64);
  const int rc = exclusive_scan(
      [values, nyu_table, nyu_len] __device__(int64_t i) {
        bool bad = false;
        return io_line_width(io_remap(values[i], nyu_table, nyu_len, &bad));
      },
      [off] __device__(int64_t i, int v) { off[i] = v; }, n, total, sws, sbytes, stream);
  if (rc != SG_OK) return rc;
  decimal_lines_kernel<<<io_grid(n), kIoBlock, 0, stream>>>(values, n, nyu_table, nyu_len, off, total, text_capacity, text,
                                                           meta);
  return check_launch("sg_decimal_lines");
}

int sg_panoptic_kitti_words(const uint32_t *words, int64_t n, const int32_t *lut, int lut_len, uint32_t *out,
                            uint64_t *missing, uint64_t *missing_host, sg_stream_t stream_) {
  SG_REQUIRE(n >= 0 && lut != nullptr && lut_len > 0 && lut_len <= 65536 && missing && missing_host &&
                 (n == 0 || (words && out)),
             "sg_panoptic_kitti_words: bad arguments");
  int32_t *host = pinned_words();
  SG_REQUIRE(host != nullptr, "sg_panoptic_kitti_words: no pinned host words");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(missing, 0, 8, stream);
  hipMemsetAsync(missing + 1, 0xFF, 8, stream);
  const bool vec = aligned16(words) && aligned16(out);
  if (n)
    panoptic_words_kernel<<<io_grid((n + 3) / 4), kIoBlock, 0, stream>>>(words, n, vec, lut, lut_len, out,
                                                                        reinterpret_cast<unsigned long long *>(missing));
  const int rc = check_launch("sg_panoptic_kitti_words");
  if (rc != SG_OK) return rc;
  uint64_t *h = reinterpret_cast<uint64_t *>(host);
  if (hipMemcpyAsync(h, missing, 16, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) {
    set_error("sg_panoptic_kitti_words: read-back failed");
    return SG_ERR_LAUNCH;
  }
  missing_host[0] = h[0];
  missing_host[1] = h[0] ? h[1] >> 16 : ~0ULL;
  missing_host[2] = h[0] ? h[1] & 0xFFFF : ~0ULL;
  if (h[0]) {
    set_error("sg_panoptic_kitti_words: %llu points whose class has no table entry (first: point %llu, class %llu)",
              static_cast<unsigned long long>(h[0]), static_cast<unsigned long long>(missing_host[1]),
              static_cast<unsigned long long>(missing_host[2]));
    return SG_ERR_UNSUPPORTED;
  }
  return SG_OK;
}

size_t sg_parse_decimal_lines_workspace_bytes(int64_t nbytes) {
  return align_up(scan_workspace_bytes(nbytes > 0 ? nbytes : 1)) + 512;
}

int sg_parse_decimal_lines(const uint8_t *text, int64_t nbytes, int64_t *values, int64_t capacity, int64_t *meta,
                           void *ws, size_t ws_bytes, sg_stream_t stream_) {
  SG_REQUIRE(nbytes >= 0 && nbytes < (1LL << 31) && capacity >= 0 && meta != nullptr &&
                 (nbytes == 0 || (text != nullptr && (capacity == 0 || values != nullptr))),
             "sg_parse_decimal_lines: bad arguments (%lld bytes)", static_cast<long long>(nbytes));
  SG_REQUIRE(ws != nullptr && ws_bytes >= sg_parse_decimal_lines_workspace_bytes(nbytes),
             "sg_parse_decimal_lines: workspace too small");
  hipStream_t stream = as_stream(stream_);
  hipMemsetAsync(meta, 0, 2 * sizeof(int64_t), stream);
  if (nbytes == 0) return check_launch("sg_parse_decimal_lines");
  Workspace a(ws, ws_bytes);
  const size_t sbytes = scan_workspace_bytes(nbytes);
  void *sws = a.take<char>(sbytes);
  int32_t *total = a.take<int32_t>(64);
  // the exclusive count of newlines in front of a line's first byte is the line's number
  const int rc = exclusive_scan(
      [text] __device__(int64_t i) { return text[i] == '\n' ? 1 : 0; },
      [text, nbytes, values, capacity, meta] __device__(int64_t i, int line) {
        if (i != 0 && text[i - 1] != '\n') return;
        int64_t v = 0;
        if (line < capacity && io_parse_line(text, i, nbytes, &v))
          values[line] = v;
        else
          atomicAdd(reinterpret_cast<unsigned long long *>(meta + 1), 1ULL);
      },
      nbytes, total, sws, sbytes, stream);
  if (rc != SG_OK) return rc;
  parse_lines_finish_kernel<<<1, 1, 0, stream>>>(text, nbytes, total, meta);
  return check_launch("sg_parse_decimal_lines");
}

int sg_parse_mask_text(const uint8_t *text, int64_t nbytes, uint8_t *flags, uint32_t *bits, int64_t *meta,
                       sg_stream_t stream_) {
  SG_REQUIRE(nbytes >= 0 && nbytes < (1LL << 32) && meta != nullptr && (nbytes == 0 || text != nullptr),
             "sg_parse_mask_text: bad arguments (%lld bytes)", static_cast<long long>(nbytes));
  SG_REQUIRE(nbytes == 0 || (aligned16(text) && aligned16(flags)), "sg_parse_mask_text: text and flags must be 16-byte aligned");
  hipStream_t stream = as_stream(stream_);
  const int64_t n_points = (nbytes + 1) / 2;
  hipMemsetAsync(meta, 0, 2 * sizeof(int64_t), stream);
  if (nbytes)
    parse_mask_kernel<<<io_grid((n_points + 31) / 32), kIoBlock, 0, stream>>>(text, nbytes, n_points, flags, bits, meta);
  return check_launch("sg_parse_mask_text");
}

}  // extern "C"
