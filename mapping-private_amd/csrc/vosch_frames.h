// vosch_frames.h -- host arithmetic of the normals / RSD / GRSD front (one frame or a batch):
// the prefixes that concatenate the frames' points, search cells, centroids and rows, the frame
// of a concatenated index, each frame's radius-search grid and the composite (frame | cell)
// sort key with its capacity checks.  Plain C++: the kernels (vosch_front.hip), the launch code
// (capi_vosch.hip) and a host check (tests/vosch_frames_check.cpp) include it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define C3H_VF_HD __host__ __device__
#else
#define C3H_VF_HD
#endif

namespace c3h {

constexpr int kVfMaxFrames = 64;                     // frames of one batch (c3h_set_batch's limit)
constexpr int64_t kVfMaxCells = (int64_t)1 << 27;    // search cells of one frame (c3h_compute_normals' limit)
constexpr int64_t kVfMaxPoints = ((int64_t)1 << 32) - 1;  // points of one batch: positions are uint32

enum { kVfOk = 0, kVfErrCells = -1, kVfErrKey = -2, kVfErrPoints = -3, kVfErrFrames = -4 };

// ---- prefixes ------------------------------------------------------------------------------
// pre[0] = 0, pre[f + 1] = pre[f] + n[f]: frame f owns [pre[f], pre[f + 1]) of the concatenation
// (empty frames own nothing).  Returns the total.
inline int64_t vf_prefix(const int64_t* n, int nf, int64_t* pre) {
  pre[0] = 0;
  for (int f = 0; f < nf; ++f) pre[f + 1] = pre[f] + n[f];
  return pre[nf];
}

// The frame of concatenated index i (0 <= i < pre[nf]): the f with pre[f] <= i < pre[f + 1].
// Empty frames are passed over wherever they sit, since no index is theirs.
C3H_VF_HD inline int vf_frame_of(const int64_t* pre, int nf, int64_t i) {
  int lo = 0, hi = nf;  // the answer is in [lo, hi): pre[lo] <= i < pre[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pre[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ---- a frame's radius-search grid ------------------------------------------------------------
// Cells of `cell` metres over the frame's voxel box [min_b, max_b] * leaf with one cell of margin
// below and two above.  The only copy of this arithmetic: every search grid comes from here.
struct VfGrid {
  float origin[3];
  float cell, inv_cell;
  int dim[3];
  int64_t ncell;
};
inline int vf_nbr_grid(const int32_t min_b[3], const int32_t max_b[3], float leaf, float cell, VfGrid* g) {
  g->cell = cell;
  g->inv_cell = 1.0f / cell;
  for (int ax = 0; ax < 3; ++ax) {
    const double lo = (double)min_b[ax] * leaf, hi = (double)(max_b[ax] + 1) * leaf;
    g->origin[ax] = (float)(lo - cell);
    g->dim[ax] = (int)std::ceil((hi - lo) / cell) + 3;
  }
  g->ncell = (int64_t)g->dim[0] * g->dim[1] * g->dim[2];
  return g->ncell > kVfMaxCells ? kVfErrCells : kVfOk;
}
// cells a query visits per axis side: ceil(radius / cell), at least 1
inline int vf_reach(float radius, float inv_cell) {
  const int r = (int)std::ceil(radius * inv_cell);
  return r > 1 ? r : 1;
}

// ---- the composite sort key --------------------------------------------------------------------
// key = frame << cell_bits | cell, sorted on its low cell_bits + frame_bits bits by one stable
// radix sort: per frame the order is cell order, then input order.  The
// all-ones cell value marks a point that is in no cell (dropped by the voxeliser), so it sorts
// behind the frame's cells; cell_bits therefore holds the value
// max_cells itself.  Keys are 32-bit words when they fit, else 64-bit.
struct VfKey {
  int cell_bits, frame_bits, bits;
  int wide;  // 1: 64-bit keys
};
C3H_VF_HD inline int vf_bits(uint64_t v) {  // bits that hold the values 0 .. v
  int b = 1;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}
inline int vf_key(int64_t max_cells, int nf, int64_t npoints, VfKey* k) {
  if (nf < 1 || nf > kVfMaxFrames) return kVfErrFrames;
  if (max_cells < 0 || max_cells > kVfMaxCells) return kVfErrCells;
  if (npoints < 0 || npoints > kVfMaxPoints) return kVfErrPoints;
  k->cell_bits = vf_bits((uint64_t)max_cells);
  k->frame_bits = vf_bits((uint64_t)(nf - 1));
  k->bits = k->cell_bits + k->frame_bits;
  if (k->bits > 64) return kVfErrKey;
  k->wide = k->bits > 32;
  return kVfOk;
}
C3H_VF_HD inline uint64_t vf_no_cell(int cell_bits) { return ((uint64_t)1 << cell_bits) - 1; }
C3H_VF_HD inline uint64_t vf_make_key(int frame, uint64_t cell, int cell_bits) { return (uint64_t)frame << cell_bits | cell; }
C3H_VF_HD inline int vf_key_frame(uint64_t key, int cell_bits) { return (int)(key >> cell_bits); }
C3H_VF_HD inline uint64_t vf_key_cell(uint64_t key, int cell_bits) { return key & vf_no_cell(cell_bits); }

// ---- the subdivisions of a frame -----------------------------------------------------------------
// extractGRSDSignature21's counts (grsd_colorCHLAC_tools.hpp:150-162; grsd_frames in capi.hip):
// sb and the row count H; H = 0 for the reference's silent-empty cases.
inline int64_t vf_subdivisions(const int32_t div_b[3], int32_t subdiv, const int32_t offset[3], int32_t sb[3],
                               float* inv_s_out) {
  sb[0] = sb[1] = sb[2] = 0;
  *inv_s_out = 0.0f;
  if (subdiv > 0) {
    const float inv_s = 1.0 / subdiv;
    *inv_s_out = inv_s;
    if (div_b[0] <= offset[0] || div_b[1] <= offset[1] || div_b[2] <= offset[2]) return 0;
    for (int a = 0; a < 3; ++a) sb[a] = (int)ceilf((div_b[a] - offset[a]) * inv_s);
    return (int64_t)sb[0] * sb[1] * sb[2];
  }
  if (subdiv < 0) return 0;
  sb[0] = sb[1] = sb[2] = 1;
  return 1;
}

}  // namespace c3h
