// pc2_layout.h -- sensor_msgs/PointCloud2 messages read in place by the batched voxeliser
// (c3h_run_pointcloud2_frames): the load plan of a call's record layout, the point index ->
// byte offset mapping of an organised message, and the extraction of the four FLOAT32 words
// (x, y, z, rgb bits) of a record.  Plain C++: the kernels (voxelize.hip), the launch code
// (capi_batch.hip) and a host check (tests/pc2_layout_check.cpp) include it.  Memory is reached
// through an accessor type (ld16 / ld4 / ld1 at a byte offset from the message's data[0]),
// so the host check runs the very loads the kernels issue and sees every byte they touch.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define C3H_PC2_HD __host__ __device__
#define C3H_PC2_UNROLL _Pragma("unroll")
#else
#define C3H_PC2_HD
#define C3H_PC2_UNROLL
#endif

namespace c3h {

// ---- the message ----------------------------------------------------------------------
// height rows of row_step bytes, the last one only width * point_step long (with one row or
// none row_step is not read at all, as c3h_voxelize_pointcloud2 has it)
C3H_PC2_HD inline uint64_t pc2_msg_bytes(uint32_t height, uint32_t width, uint32_t point_step, uint32_t row_step) {
  if (height == 0 || width == 0) return 0;
  return (uint64_t)(height - 1) * row_step + (uint64_t)width * point_step;
}
// a message without row padding: point i's record starts at i * point_step
C3H_PC2_HD inline bool pc2_flat(uint32_t height, uint32_t width, uint32_t point_step, uint32_t row_step) {
  return height <= 1 || (uint64_t)row_step == (uint64_t)width * point_step;
}

// ---- point index -> byte offset ---------------------------------------------------------
// Row of point i (i < 2^24) of a message `width` points wide, without a division: with
// L = ceil(log2 width) and magic = ceil(2^(24 + L) / width) <= 2^25,
//   i / width = floor(i * magic / 2^(24 + L)) = mulhi32(i << 8, magic) >> L.
// Exact: magic * width = 2^(24 + L) + e with 0 <= e < width, so i * magic / 2^(24 + L) exceeds
// i / width by i * e / (width * 2^(24 + L)) < 2^24 * width / (width * 2^24 * width) = 1 / width,
// the smallest gap from i / width to the next integer.
struct Pc2Frame {
  uint32_t width, row_step;
  uint32_t magic;  // 0: flat
  uint32_t shift;  // L
};
C3H_PC2_HD inline Pc2Frame pc2_frame(uint32_t height, uint32_t width, uint32_t point_step, uint32_t row_step) {
  Pc2Frame f{width, row_step, 0u, 0u};
  if (pc2_flat(height, width, point_step, row_step) || width == 0) return f;
  uint32_t L = 0;
  while (((uint64_t)1 << L) < width) ++L;
  const uint64_t p = (uint64_t)1 << (24 + L);
  f.magic = (uint32_t)((p + width - 1) / width);
  f.shift = L;
  return f;
}
C3H_PC2_HD inline uint32_t pc2_row(uint32_t i, uint32_t magic, uint32_t shift) {
  return (uint32_t)(((uint64_t)(i << 8) * magic) >> 32) >> shift;
}
C3H_PC2_HD inline uint64_t pc2_offset(uint32_t i, const Pc2Frame& f, uint32_t point_step) {
  if (f.magic == 0) return (uint64_t)i * point_step;
  const uint32_t row = pc2_row(i, f.magic, f.shift), col = i - row * f.width;
  return (uint64_t)row * f.row_step + (uint64_t)col * point_step;
}

// ---- the plan of a call -------------------------------------------------------------------
// VEC16: every 16-byte piece of the record that holds a wanted field is one 16-byte load (the
//        Kinect / PCL PointXYZRGB record, step 32 with rgb at 16: two pieces; the packed float4
//        record: one); a field is dword sel[k] of the pieces laid end to end.  Little-endian,
//        point_step and every row_step read multiples of 16, bases 16-byte aligned, offsets
//        multiples of 4, the wanted fields in at most two pieces (more: DWORD loads less).
// DWORD: one 4-byte load per field.  Little-endian, everything 4-byte aligned.
// BYTES: every field byte by byte (big-endian messages, odd offsets or steps).
// No form reads a byte outside a record: pieces lie inside it because point_step is a
// multiple of 16, the other forms read field bytes only.
enum : int32_t { kPc2Vec16 = 0, kPc2Dword = 1, kPc2Bytes = 2 };
struct Pc2Plan {
  int32_t form;
  int32_t npiece;       // VEC16: 1 or 2
  uint32_t point_step;
  int32_t big;
  int32_t off[4];       // byte offsets of x, y, z, rgb (rgb < 0: absent, read as 0)
  int32_t piece[2];     // VEC16: byte offsets of the pieces
  int32_t sel[4];       // VEC16: the field's dword among the pieces' 4 * npiece (-1: absent)
};

// what the plan needs to know of the messages: the OR of every base address, and of every
// row_step that is read (messages with row padding), over the frames that hold points
C3H_PC2_HD inline Pc2Plan pc2_plan(uint32_t point_step, const int32_t off[4], int big, uint64_t base_or,
                                   uint32_t row_step_or) {
  Pc2Plan p{};
  p.point_step = point_step;
  p.big = big ? 1 : 0;
  for (int k = 0; k < 4; ++k) p.off[k] = off[k] < 0 ? -1 : off[k];
  p.piece[0] = p.piece[1] = 0;
  for (int k = 0; k < 4; ++k) p.sel[k] = -1;
  uint32_t al = (uint32_t)(base_or & 15u) | (row_step_or & 15u) | (point_step & 15u);
  uint32_t fo = 0;
  for (int k = 0; k < 4; ++k)
    if (off[k] >= 0) fo |= (uint32_t)off[k];
  p.form = kPc2Bytes;
  if (big || ((al | fo) & 3u)) return p;
  p.form = kPc2Dword;
  if (al & 15u) return p;
  int np = 0, piece[2] = {0, 0};
  for (int k = 0; k < 4; ++k) {
    if (off[k] < 0) continue;
    const int pc = off[k] & ~15;
    int j = 0;
    while (j < np && piece[j] != pc) ++j;
    if (j == np) {
      if (np == 2) return p;  // a third piece: DWORD
      piece[np++] = pc;
    }
    p.sel[k] = 4 * j + ((off[k] & 15) >> 2);
  }
  p.form = kPc2Vec16;
  p.npiece = np;
  p.piece[0] = piece[0];
  p.piece[1] = piece[1];
  return p;
}

// ---- loading and extracting a record ----------------------------------------------------
// Raw: what a lane holds between the loads of a round and their use
template <int kForm, int kNP>
struct Pc2Raw {
  uint32_t w[kForm == kPc2Vec16 ? 4 * kNP : 4];
};

C3H_PC2_HD inline uint32_t pc2_bytes_word(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int big) {
  return big ? (b0 << 24 | b1 << 16 | b2 << 8 | b3) : (b3 << 24 | b2 << 16 | b1 << 8 | b0);
}

// the record at byte offset o of the message behind m
template <int kForm, int kNP, class Mem>
C3H_PC2_HD inline Pc2Raw<kForm, kNP> pc2_load(const Mem& m, uint64_t o, const Pc2Plan& L) {
  Pc2Raw<kForm, kNP> r;
  if constexpr (kForm == kPc2Vec16) {
    C3H_PC2_UNROLL
    for (int j = 0; j < kNP; ++j) m.ld16(o + (uint32_t)L.piece[j], r.w + 4 * j);
  } else if constexpr (kForm == kPc2Dword) {
    C3H_PC2_UNROLL
    for (int k = 0; k < 4; ++k) r.w[k] = L.off[k] >= 0 ? m.ld4(o + (uint32_t)L.off[k]) : 0u;
  } else {
    C3H_PC2_UNROLL
    for (int k = 0; k < 4; ++k) {
      if (L.off[k] >= 0) {
        const uint64_t q = o + (uint32_t)L.off[k];
        const uint32_t b0 = m.ld1(q), b1 = m.ld1(q + 1), b2 = m.ld1(q + 2), b3 = m.ld1(q + 3);
        r.w[k] = pc2_bytes_word(b0, b1, b2, b3, L.big);
      } else {
        r.w[k] = 0u;
      }
    }
  }
  return r;
}

// the four words x, y, z, rgb of a loaded record (the index into the pieces is the same for
// every lane: selects on a scalar condition, no indexed register access)
template <int kForm, int kNP>
C3H_PC2_HD inline void pc2_extract(const Pc2Raw<kForm, kNP>& r, const Pc2Plan& L, uint32_t out[4]) {
  if constexpr (kForm == kPc2Vec16) {
    C3H_PC2_UNROLL
    for (int k = 0; k < 4; ++k) {
      uint32_t v = L.sel[k] < 0 ? 0u : r.w[0];
    C3H_PC2_UNROLL
      for (int d = 1; d < 4 * kNP; ++d) v = L.sel[k] == d ? r.w[d] : v;
      out[k] = v;
    }
  } else {
    C3H_PC2_UNROLL
    for (int k = 0; k < 4; ++k) out[k] = r.w[k];
  }
}

}  // namespace c3h
