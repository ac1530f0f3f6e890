// feat_rows.h -- index arithmetic of the feature-rows front (c3h_run_feature_frames):
// the canvas row <-> frame row mapping, the row-block / alignment plan of the front kernel's
// stream, and the three exist rules of SearchObj::setData's callers.  Plain C++: the kernel
// (search.hip), its launch code and a host check (tests/feat_rows_check.cpp) include it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define C3H_FR_HD __host__ __device__
#else
#define C3H_FR_HD
#endif

namespace c3h {

// ---- canvas row <-> frame row ---------------------------------------------------------
// A frame of sb[0] x sb[1] x sb[2] subdivisions sits at the origin of a canvas of cb[] (sb <= cb
// per axis).  Rows are h = x + y * xn + z * xn * yn in the counts of their own layout.
// Canvas row c -> the frame's row, or -1 when (x, y, z) lies outside the frame's counts.
C3H_FR_HD inline int64_t fr_canvas_to_frame(int64_t c, const int cb[3], const int sb[3]) {
  const int x = (int)(c % cb[0]), y = (int)((c / cb[0]) % cb[1]), z = (int)(c / ((int64_t)cb[0] * cb[1]));
  if (x >= sb[0] || y >= sb[1] || z >= sb[2]) return -1;
  return x + (int64_t)sb[0] * (y + (int64_t)sb[1] * z);
}
// Frame row h (0 <= h < sb[0] * sb[1] * sb[2]) -> its canvas row.
C3H_FR_HD inline int64_t fr_frame_to_canvas(int64_t h, const int cb[3], const int sb[3]) {
  const int x = (int)(h % sb[0]), y = (int)((h / sb[0]) % sb[1]), z = (int)(h / ((int64_t)sb[0] * sb[1]));
  return x + (int64_t)cb[0] * (y + (int64_t)cb[1] * z);
}

// ---- row blocks ------------------------------------------------------------------------
// A workgroup stages a block of consecutive frame rows in LDS as one flat span of floats:
// as many rows as fit kFrStageFloats, at most one per thread of the workgroup (dim 21: 256
// rows, 137: 59, 981: 8).  A row longer than the stage has no plan (fr_block_rows 0).
constexpr int kFrStageFloats = 8192;  // 32 KiB
constexpr int kFrMaxRows = 256;
C3H_FR_HD inline int fr_block_rows(int dim) {
  if (dim < 1 || dim > kFrStageFloats) return 0;
  const int r = kFrStageFloats / dim;
  return r < kFrMaxRows ? r : kFrMaxRows;
}

// Element e of a block's span (e < kFrStageFloats) -> its row e / dim, as a multiply-high by
// fr_div_magic(dim) = floor(2^32 / dim) + 1: exact while e * dim < 2^32 (here < 2^26).
C3H_FR_HD inline uint32_t fr_div_magic(int dim) { return dim > 1 ? (uint32_t)(0x100000000ull / (uint32_t)dim) + 1u : 0u; }
C3H_FR_HD inline uint32_t fr_div(int e, int dim, uint32_t magic) {
  return dim > 1 ? (uint32_t)(((uint64_t)(uint32_t)e * magic) >> 32) : (uint32_t)e;
}

// The span of n floats starting at word address w (byte address / 4; rows of odd dim are not
// 16-byte aligned, so the span is cut instead of the rows): `head` single words up to the next
// 16-byte boundary, `nvec` aligned 16-byte vectors, `tail` single words.  In LDS the span is
// stored from word `pad` on, which puts the vectors at 16-byte aligned LDS addresses too.
struct FrSpan {
  int head, nvec, tail, pad;
};
C3H_FR_HD inline FrSpan fr_span(uint64_t w, int n) {
  FrSpan s;
  const int to_boundary = (int)((4 - (w & 3)) & 3);
  s.head = to_boundary < n ? to_boundary : n;
  s.nvec = (n - s.head) / 4;
  s.tail = n - s.head - 4 * s.nvec;
  s.pad = (4 - s.head) & 3;
  return s;
}
constexpr int kFrStageWords = kFrStageFloats + 4;  // the stage with its pad

// ---- exist rules -------------------------------------------------------------------------
// exist_voxel_num of a caller's feature row, with the reference's float / int arithmetic:
// C3H_EXIST_C3HLAC (0) setC3HLAC: (f0 + f1) * 2 + 0.001 (search_c3_hlac.h:60-61);
// C3H_EXIST_VOSCH (1) setVOSCH / setConVOSCH: (f20 + f21) * 2 + 0.001 (search_new.h:41-43);
// C3H_EXIST_GRSD (2) setGRSD: an int accumulating f0 .. f19 one float add at a time, then / 26
// (search_new.h:69-74).
C3H_FR_HD inline int32_t fr_exist_pair(float a, float b) {
  const float t = (a + b) * 2.0f;
  return (int32_t)((double)t + 0.001);
}
C3H_FR_HD inline int32_t fr_exist_grsd(const float* f) {
  int32_t e = 0;
  for (int i = 0; i < 20; ++i) e = (int32_t)((float)e + f[i]);
  return e / 26;
}
C3H_FR_HD inline int32_t fr_exist_rule(const float* f, int rule) {
  if (rule == 2) return fr_exist_grsd(f);
  const int i0 = rule == 1 ? 20 : 0;
  return fr_exist_pair(f[i0], f[i0 + 1]);
}
// the smallest row a rule reads (c3h_set_features' dim minimums)
C3H_FR_HD inline int fr_exist_min_dim(int rule) { return rule == 1 ? 22 : (rule == 2 ? 20 : 2); }

}  // namespace c3h
