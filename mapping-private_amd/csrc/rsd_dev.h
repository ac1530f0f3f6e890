// rsd_dev.h -- the arithmetic of the normals, the RSD radii and the GRSD transitions as device
// functions the kernels of the front (vosch_front.hip, where the algorithm is described) call,
// whichever of them serves a point or a voxel.  The library is built
// with -ffp-contract=off: every product and sum below rounds where it is written.
#pragma once
#include "c3h_internal.h"

namespace c3h {

// the points c3h_voxelize kept (voxelize.hip point_valid: finite, z < z_limit)
__device__ __forceinline__ bool pt_kept(const NbrGrid& g, const float4& p) {
  return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && p.z < g.z_limit;
}

__device__ __forceinline__ bool cell_of(const NbrGrid& g, const float4& p, int c[3]) {
  const float v[3] = {p.x, p.y, p.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t = floorf((v[a] - g.origin[a]) * g.inv_cell);
    if (!(t >= 0.0f && t < (float)g.dim[a])) return false;
    c[a] = (int)t;
  }
  return true;
}

// the cell a query's neighbour walk starts from (no range check: cells outside are skipped)
__device__ __forceinline__ void query_cell(const NbrGrid& g, const float4& q, int c[3]) {
  const float v[3] = {q.x, q.y, q.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = (int)floorf((v[a] - g.origin[a]) * g.inv_cell);
}

// float squared distance, as FLANN compares it
__device__ __forceinline__ float pair_d2(const float4& p, const float4& q) {
  const float ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
  return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}

// visit every grid point within sqrt(r2) of q (float squared distance < r2, strict as
// FLANN's radius result set), in cell order then input order
template <class F>
__device__ __forceinline__ void for_neighbours(const NbrGrid& g, const float4& q, float r2, int reach, F&& f) {
  int c[3];
  query_cell(g, q, c);
  for (int dz = -reach; dz <= reach; ++dz) {
    const int z = c[2] + dz;
    if (z < 0 || z >= g.dim[2]) continue;
    for (int dy = -reach; dy <= reach; ++dy) {
      const int y = c[1] + dy;
      if (y < 0 || y >= g.dim[1]) continue;
      for (int dx = -reach; dx <= reach; ++dx) {
        const int x = c[0] + dx;
        if (x < 0 || x >= g.dim[0]) continue;
        const uint32_t cell = (uint32_t)(x + g.dim[0] * (y + g.dim[1] * z));
        const uint32_t e = g.cend[cell];
        for (uint32_t s = g.cstart[cell]; s < e; ++s) {
          const uint32_t j = g.sorted[s];
          const float4 p = g.pts[j];
          const float d2 = pair_d2(p, q);
          if (d2 < r2) f(j, p, d2);
        }
      }
    }
  }
}

// eigen decomposition of a symmetric 3 x 3 matrix (cyclic Jacobi, double): w ascending,
// V columns the eigenvectors
static __device__ void sym3_eigen(double A[3][3], double w[3], double V[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    if (off == 0.0) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {  // A = J^T A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int o[3] = {0, 1, 2};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (A[o[j]][o[j]] < A[o[i]][o[i]]) {
        const int t = o[i];
        o[i] = o[j];
        o[j] = t;
      }
  double W[3][3];
  for (int i = 0; i < 3; ++i) {
    w[i] = A[o[i]][o[i]];
    for (int k = 0; k < 3; ++k) W[k][i] = V[k][o[i]];
  }
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) V[k][i] = W[k][i];
}

// ---- normals ------------------------------------------------------------------------------
// s: n, x, y, z, xx, xy, xz, yy, yz, zz of the neighbours, added in visiting order
__device__ __forceinline__ void nrm_accum(double s[10], const float4& p) {
  const double x = p.x, y = p.y, z = p.z;
  s[0] += 1;
  s[1] += x;
  s[2] += y;
  s[3] += z;
  s[4] += x * x;
  s[5] += x * y;
  s[6] += x * z;
  s[7] += y * y;
  s[8] += y * z;
  s[9] += z * z;
}

// covariance -> smallest-eigenvalue eigenvector, flipped towards the viewpoint, curvature;
// < 3 neighbours -> NaN (PCL)
__device__ __forceinline__ float4 nrm_from_sums(const double s[10], const float4& q, float vx, float vy, float vz) {
  const float nan = __int_as_float(0x7fc00000);
  float4 res = make_float4(nan, nan, nan, nan);
  if (s[0] >= 3) {
    const double n = s[0], mx = s[1] / n, my = s[2] / n, mz = s[3] / n;
    double A[3][3] = {{s[4] / n - mx * mx, s[5] / n - mx * my, s[6] / n - mx * mz},
                      {0, s[7] / n - my * my, s[8] / n - my * mz},
                      {0, 0, s[9] / n - mz * mz}};
    A[1][0] = A[0][1];
    A[2][0] = A[0][2];
    A[2][1] = A[1][2];
    double w[3], V[3][3];
    sym3_eigen(A, w, V);
    double nx = V[0][0], ny = V[1][0], nz = V[2][0];
    const double nl = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= nl;
    ny /= nl;
    nz /= nl;
    // flipNormalTowardsViewpoint
    if ((vx - (double)q.x) * nx + (vy - (double)q.y) * ny + (vz - (double)q.z) * nz < 0) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    const double tr = w[0] + w[1] + w[2];
    res = make_float4((float)nx, (float)ny, (float)nz, (float)(tr != 0 ? w[0] / tr : 0.0));
  }
  return res;
}

// the normal of one point by the per-pair gather over the grid
__device__ __forceinline__ float4 nrm_point(const NbrGrid& g, const float4& q, float r2, int reach, float vx, float vy,
                                            float vz) {
  const float nan = __int_as_float(0x7fc00000);
  if (!pt_kept(g, q)) return make_float4(nan, nan, nan, nan);
  double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for_neighbours(g, q, r2, reach, [&](uint32_t, const float4& p, float) { nrm_accum(s, p); });
  return nrm_from_sums(s, q, vx, vy, vz);
}

// ---- RSD ----------------------------------------------------------------------------------
// grsd_colorCHLAC_tools.hpp:99-118
__device__ __forceinline__ int grsd_type(float rmin, float rmax) {
  if ((double)rmin > 0.100) return 1;  // PLANE
  if ((double)rmax > 0.175) return 2;  // CYLINDER
  if ((double)rmin < 0.015) return 0;  // NOISE
  if ((double)(rmax - rmin) < 0.050) return 3;  // SPHERE
  return 4;  // EDGE
}

constexpr int kRsdSubdiv = 5;  // RSDEstimation defaults: nr_subdiv 5, plane_radius 0.2

// PCL's computeRSD for the centroid q over the grid's points within max_dist of it
__device__ __forceinline__ void rsd_point(const NbrGrid& g, const float4* __restrict__ nrm, const float4& q,
                                          float max_dist, int reach, float2* radii_out, int32_t* type_out) {
  const double kPi = 3.14159265358979323846;
  const float r2 = max_dist * max_dist;
  // the nearest neighbour (ties: the lower point index) and the neighbour count
  uint32_t best = 0xffffffffu;
  float bd = 0.0f;
  int cnt = 0;
  for_neighbours(g, q, r2, reach, [&](uint32_t j, const float4&, float d2) {
    ++cnt;
    if (best == 0xffffffffu || d2 < bd || (d2 == bd && j < best)) {
      best = j;
      bd = d2;
    }
  });
  float rmin = 0.0f, rmax = 0.0f;
  if (cnt >= 2) {
    double mn[kRsdSubdiv], mx[kRsdSubdiv];
    mn[0] = mx[0] = 0.0;
    for (int d = 1; d < kRsdSubdiv; ++d) {
      mn[d] = 1.7976931348623157e308;
      mx[d] = -1.7976931348623157e308;
    }
    const float4 pb = g.pts[best];
    const float4 nb = nrm[best];
    for_neighbours(g, q, r2, reach, [&](uint32_t j, const float4& p, float) {
      if (j == best) return;
      const float4 ni = nrm[j];
      double cosine = (double)__fadd_rn(__fadd_rn(__fmul_rn(ni.x, nb.x), __fmul_rn(ni.y, nb.y)), __fmul_rn(ni.z, nb.z));
      if (cosine > 1) cosine = 1;
      if (cosine < -1) cosine = -1;
      double angle = acos(cosine);
      if (angle > kPi / 2) angle = kPi - angle;
      const float ex = p.x - pb.x, ey = p.y - pb.y, ez = p.z - pb.z;
      const double dist = sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez)));
      if (dist > max_dist) return;
      int bin = (int)floor(kRsdSubdiv * dist / max_dist);
      if (bin > kRsdSubdiv - 1) bin = kRsdSubdiv - 1;
      if (mn[bin] > angle) mn[bin] = angle;
      if (mx[bin] < angle) mx[bin] = angle;
    });
    double aa = 0, ad = 0, xa = 0, xd = 0;
    for (int d = 0; d < kRsdSubdiv; ++d)
      if (mx[d] >= 0) {
        const double f = (d + 0.5) * max_dist / kRsdSubdiv;
        aa += mn[d] * mn[d];
        ad += mn[d] * f;
        xa += mx[d] * mx[d];
        xd += mx[d] * f;
      }
    const double plane = 0.2;
    float a = (float)(aa == 0 ? plane : fmin(ad / aa, plane));
    float b = (float)(xa == 0 ? plane : fmin(xd / xa, plane));
    a = (float)(a * 1.1);
    b = (float)(b * 0.9);
    rmin = a < b ? a : b;
    rmax = a < b ? b : a;
  }
  *radii_out = make_float2(rmin, rmax);
  *type_out = grsd_type(rmin, rmax);
}

// ---- GRSD ---------------------------------------------------------------------------------
// One occupied voxel (centroid c of a): its type against the 26 neighbour voxels (EMPTY where
// unoccupied), int atomics into its subdivision's 6 x 6 matrix.  leaf_of(linear voxel index) =
// the voxel's position in the downsampled cloud, or < 0 where the voxel is empty.
template <class LeafOf>
__device__ __forceinline__ void grsd_voxel(const GrsdArgs& a, int64_t c, LeafOf&& leaf_of) {
  const float4 p = a.cent[c];
  const float v[3] = {p.x, p.y, p.z};
  int64_t h = 0;
  if (a.hist1 == 0) {  // hist_idx (grsd_colorCHLAC_tools.hpp:245-258)
    int ijk[3];
    bool ok = true;
    for (int ax = 0; ax < 3; ++ax) {
      const int t = (int)floorf(__fdiv_rn(v[ax], a.leaf)) - a.min_b[ax] - a.off[ax];
      ok = ok && t >= 0;
      ijk[ax] = (int)floorf((float)t * a.inv_s);
      ok = ok && ijk[ax] < a.sb[ax];
    }
    if (!ok) return;
    h = ijk[0] + (int64_t)a.sb[0] * (ijk[1] + (int64_t)a.sb[1] * ijk[2]);
  }
  const int src = a.types[c];
  int base[3];
  for (int ax = 0; ax < 3; ++ax) base[ax] = (int)floorf(v[ax] * a.inv_leaf) - a.min_b[ax];
  int32_t* T = a.trans + h * 36 + src * 6;
  for (int k = 0; k < 26; ++k) {  // relative_coordinates, then their negatives
    const int kk = k % 13, sg = k < 13 ? 1 : -1;
    const int rdx = kk <= 8 ? kk / 3 - 1 : (kk <= 11 ? kk - 10 : -1);
    const int rdy = kk <= 8 ? kk % 3 - 1 : (kk <= 11 ? -1 : 0);
    const int rdz = kk <= 8 ? -1 : 0;
    const int x = base[0] + sg * rdx, y = base[1] + sg * rdy, z = base[2] + sg * rdz;
    int nt = 5;  // EMPTY
    if (x >= 0 && y >= 0 && z >= 0 && x < a.div_b[0] && y < a.div_b[1] && z < a.div_b[2]) {
      const int32_t li = leaf_of(x + (int64_t)a.div_b[0] * (y + (int64_t)a.div_b[1] * z));
      if (li >= 0) nt = a.types[li];
    }
    atomicAdd(&T[nt], 1);
  }
}

// feature bin b (0 .. 19) -> its cell (i, j >= i) of the 6 x 6 matrix: the upper triangle in
// row order (grsd_colorCHLAC_tools.hpp:277-283)
__device__ __forceinline__ int grsd_bin_cell(int b) {
  int i = 0, j = 0, k = 0;
  for (i = 0; i < 6; ++i) {
    if (b < k + (6 - i)) {
      j = i + (b - k);
      break;
    }
    k += 6 - i;
  }
  return i * 6 + j;
}

}  // namespace c3h
