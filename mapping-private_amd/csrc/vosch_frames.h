// vosch_frames.h -- host arithmetic of the normals / RSD / GRSD front (one frame or a batch):
// the prefixes that concatenate the frames' points, search cells, centroids and rows, the frame
// of a concatenated index, each frame's radius-search grid and the composite (frame | cell)
// sort key with its capacity checks; and of the batched voxel head in front of it (voxelize.hip
// vh_*): its composite (frame | voxel) key, the record the device leaves of a frame and the host's
// decision on it.  Plain C++: the kernels (vosch_front.hip, voxelize.hip), the launch code
// (capi_vosch.hip) and the host checks (tests/vosch_frames_check.cpp, tests/vox_head_check.cpp)
// include it.
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

// A wide RSD radius (large leaves: leaf sqrt(3)/2 > 4 x the normal radius) gets a search grid of
// its own radius
inline bool vf_rsd_wide(float max_dist, float cell) { return max_dist > 4 * cell; }

// ---- the batched voxel head (voxelize.hip vh_*, capi_vosch.hip) --------------------------------
// The frames of a batch are voxelised together: a bounds pass over the concatenated points, the
// host's decision per frame (below), then one stable radix sort of (frame << voxel_bits | linear
// voxel index, point) pairs.  A run of equal keys is a voxel, its points in input order; the
// runs' ordinals are leaf-layout order (ascending voxel index), frame after frame.
constexpr int64_t kVhMaxVoxels = INT32_MAX;               // linear voxel indices are int32 (c3h_voxelize's limit)
constexpr int64_t kVhMaxFramePoints = ((int64_t)1 << 24) - 1;  // points of one frame (c3h_voxelize's limit)

// The voxel variant of vf_key: voxel_bits (VfKey::cell_bits) holds the largest div_b product of
// the batch itself, so the all-ones value is no voxel's index and sorts behind every voxel of
// its frame (a point the voxeliser drops).  The keys are always 64-bit words: sorted on the same
// bits, 32-bit words were measured level with them, so the one
// width serves every batch, up to 2^31 - 1 voxels in each of 64 frames (37 bits).
inline int vh_key(int64_t max_voxels, int nf, int64_t npoints, VfKey* k) {
  if (nf < 1 || nf > kVfMaxFrames) return kVfErrFrames;
  if (max_voxels < 0 || max_voxels > kVhMaxVoxels) return kVfErrCells;
  if (npoints < 0 || npoints > kVfMaxPoints) return kVfErrPoints;
  k->cell_bits = vf_bits((uint64_t)max_voxels);
  k->frame_bits = vf_bits((uint64_t)(nf - 1));
  k->bits = k->cell_bits + k->frame_bits;
  k->wide = 1;
  return kVfOk;
}

// What the bounds pass and the emit leave of one frame on the device, read back by the host
struct VhRec {
  int32_t mn[3], mx[3];          // min / max cell of the valid points (INT32_MAX / INT32_MIN: none)
  uint32_t beyond;               // a valid point's cell lies beyond +-2^20
  uint32_t n_occ;                // occupied voxels (runs)
  unsigned long long n_valid;    // valid points
  uint32_t n_off;                // voxels whose centroid lies in another cell
};
inline VhRec vh_rec_init() {
  VhRec r{};
  for (int a = 0; a < 3; ++a) {
    r.mn[a] = INT32_MAX;
    r.mx[a] = INT32_MIN;
  }
  return r;
}

// Why a frame of the batch fails, in the order the single-frame route (c3h_voxelize,
// c3h_compute_normals, c3h_extract_vosch / _grsd) meets the reasons: the first that holds decides.
enum VhReason {
  kVhGood = 0,
  kVhArgs,       // n < 0, or no pointer with n > 0             C3H_ERR_ARG
  kVhPoints,     // n >= 2^24                                    C3H_ERR_RANGE
  kVhBeyond,     // a valid point's cell beyond +-2^20           C3H_ERR_RANGE
  kVhNoPoint,    // no valid point                               C3H_ERR_STATE
  kVhVoxels,     // div_b product above INT32_MAX                C3H_ERR_RANGE
  kVhCells,      // more than 2^27 search cells (either grid; not where VhCall::no_grids)  C3H_ERR_RANGE
  kVhRows        // more rows than row_cap                       C3H_ERR_RANGE
};
// the C3H_ERR_* value of a reason (capi_vosch.hip asserts that they are the header's)
constexpr int vh_status(int reason) {
  switch (reason) {
    case kVhGood: return 0;
    case kVhArgs: return -1;
    case kVhNoPoint: return -3;
    default: return -5;
  }
}
// the reasons known before any point is read
inline int vh_args_reason(int64_t n, bool has_pointer) {
  if (n < 0 || (n > 0 && !has_pointer)) return kVhArgs;
  if (n > kVhMaxFramePoints) return kVhPoints;
  return kVhGood;
}
struct VhCall {          // what every frame of a call shares
  float leaf, radius;    // voxel size, normals radius (the cell of g)
  float rsd_dist;        // the RSD radius (the cell of g2 where vf_rsd_wide holds)
  int32_t subdiv, offset[3];
  int64_t row_cap;
  int32_t no_grids;      // 1: a call without normals or RSD (c3h_extract_c3_frames): no search grid is
                         //    sized and kVhCells never holds; g and g2 stay zero
};
struct VhFrameGeom {     // the host's share of a good frame
  int32_t min_b[3], max_b[3], div_b[3];
  int64_t n_valid, nvox;
  VfGrid g, g2;
  int32_t sb[3];
  int64_t H;
  float inv_s;
};
// A frame's reason and, for a good frame, its geometry.  rec: the bounds pass's record (unread
// where the arguments already fail).
inline int vh_frame_decide(int64_t n, bool has_pointer, const VhRec& rec, const VhCall& q, VhFrameGeom* out) {
  *out = VhFrameGeom{};
  const int r0 = vh_args_reason(n, has_pointer);
  if (r0 != kVhGood) return r0;
  if (rec.beyond) return kVhBeyond;
  if (rec.n_valid == 0) return kVhNoPoint;
  out->n_valid = (int64_t)rec.n_valid;
  out->nvox = 1;
  for (int a = 0; a < 3; ++a) {
    out->min_b[a] = rec.mn[a];
    out->max_b[a] = rec.mx[a];
    out->div_b[a] = rec.mx[a] - rec.mn[a] + 1;
    out->nvox *= out->div_b[a];  // (each factor < 2^21: no overflow)
  }
  if (out->nvox > kVhMaxVoxels) return kVhVoxels;
  if (!q.no_grids && vf_nbr_grid(out->min_b, out->max_b, q.leaf, q.radius, &out->g) != kVfOk) return kVhCells;
  out->g2 = out->g;
  out->H = vf_subdivisions(out->div_b, q.subdiv, q.offset, out->sb, &out->inv_s);
  if (out->H > q.row_cap) return kVhRows;
  if (!q.no_grids && out->H > 0 && vf_rsd_wide(q.rsd_dist, q.radius) &&
      vf_nbr_grid(out->min_b, out->max_b, q.leaf, q.rsd_dist, &out->g2) != kVfOk)
    return kVhCells;
  return kVhGood;
}

}  // namespace c3h
