// rsd.hip -- normals, RSD radii and GRSD transition histograms on the GPU (SURVEY.md
// 8(f)4, the VOSCH / GRSD features of color_chlac/include/color_chlac/
// grsd_colorCHLAC_tools.hpp:63-296, 832-843).
//
// Radius searches run over a dense grid of cells of the normal radius: the points are
// sorted by cell (rocPRIM radix sort of (cell, point) pairs: stable, so a cell lists its
// points in input order) and every cell keeps its [start, end) range.  A query visits
// the cells within ceil(radius / cell) of its own.
//   normals_kernel: one point per thread; double sums of the neighbours within the
//     radius (the point included, squared distances in float as FLANN compares them);
//     covariance -> smallest-eigenvalue eigenvector (Jacobi, double), flipped towards
//     the viewpoint, curvature = lambda_min / trace; < 3 neighbours -> NaN (PCL).  A
//     point the voxeliser dropped is nobody's neighbour and gets NaN.
//   rsd_kernel: one downsampled centroid per thread; PCL's computeRSD over the cloud
//     points within max(rsd_radius, leaf sqrt(3) / 2) of it: the nearest one is the
//     reference ("begin"), the others' normal angles are binned by their distance to it.
//   grsd_kernel: one occupied voxel per thread; its type against the 26 neighbour voxels
//     (EMPTY where unoccupied), int atomics into its subdivision's 6 x 6 matrix.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "c3h_internal.h"
#include "rsd_dev.h"

namespace c3h {
namespace {

__global__ void nbr_keys_kernel(NbrGrid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = g.pts[i];
    int c[3];
    keys[i] = pt_kept(g, p) && cell_of(g, p, c) ? (uint32_t)(c[0] + g.dim[0] * (c[1] + g.dim[1] * c[2])) : kNoCell;
    idx[i] = (uint32_t)i;
  }
}

__global__ void nbr_ranges_kernel(const uint32_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ cstart,
                                  uint32_t* __restrict__ cend) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t k = keys[i];
    if (k == kNoCell) continue;
    if (i == 0 || keys[i - 1] != k) cstart[k] = (uint32_t)i;
    if (i == n - 1 || keys[i + 1] != k) cend[k] = (uint32_t)(i + 1);
  }
}

__global__ void normals_kernel(NbrGrid g, float r2, int reach, float vx, float vy, float vz,
                               float4* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = nrm_point(g, g.pts[i], r2, reach, vx, vy, vz);
}

__global__ void rsd_kernel(NbrGrid g, const float4* __restrict__ nrm, const float4* __restrict__ cent,
                           int64_t nc, float max_dist, int reach, float2* __restrict__ radii,
                           int32_t* __restrict__ types) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nc; c += (int64_t)gridDim.x * blockDim.x)
    rsd_point(g, nrm, cent[c], max_dist, reach, &radii[c], &types[c]);
}

__global__ void grsd_kernel(GrsdArgs a) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < a.nc; c += (int64_t)gridDim.x * blockDim.x)
    grsd_voxel(a, c, [&](int64_t v) { return a.layout[v]; });
}

// upper-triangle bins (i <= j) of each 6 x 6 matrix, the first 20 (:277-283), times norm
__global__ void grsd_feat_kernel(const int32_t* __restrict__ trans, int64_t H, float norm, float* __restrict__ out,
                                 int stride) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < H * 20; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t h = e / 20;
    const int b = (int)(e - h * 20);
    out[h * stride + b] = (float)trans[h * 36 + grsd_bin_cell(b)] * norm;
  }
}

// [grsd (20) | c3 (117)] rows; c3 rows of empty subdivisions may be stale: exist 0 -> zeros
__global__ void vosch_concat_kernel(const float* __restrict__ grsd, const float* __restrict__ c3,
                                    const int32_t* __restrict__ exist, int64_t H, float* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < H * 137; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t h = e / 137;
    const int t = (int)(e - h * 137);
    out[e] = t < 20 ? grsd[h * 20 + t] : (exist[h] ? c3[h * 117 + (t - 20)] : 0.0f);
  }
}

int grid_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

}  // namespace

hipError_t nbr_build(NbrGrid& g, uint32_t* keys, uint32_t* keys2, uint32_t* idx, uint32_t* idx2, void* tmp,
                     size_t* tmp_bytes, hipStream_t s) {
  if (!tmp) {  // size query
    size_t b = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, b, keys, keys2, idx, idx2, (size_t)std::max<int64_t>(g.n, 1),
                                                   0, 32, s);
    *tmp_bytes = b;
    return e;
  }
  nbr_keys_kernel<<<grid_blocks(g.n), 256, 0, s>>>(g, keys, idx);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t b = *tmp_bytes;
  e = rocprim::radix_sort_pairs(tmp, b, keys, keys2, idx, idx2, (size_t)g.n, 0, 32, s);
  if (e != hipSuccess) return e;
  const int64_t ncell = (int64_t)g.dim[0] * g.dim[1] * g.dim[2];
  e = hipMemsetAsync(const_cast<uint32_t*>(g.cstart), 0, ncell * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(const_cast<uint32_t*>(g.cend), 0, ncell * 4, s);
  if (e != hipSuccess) return e;
  nbr_ranges_kernel<<<grid_blocks(g.n), 256, 0, s>>>(keys2, g.n, const_cast<uint32_t*>(g.cstart),
                                                    const_cast<uint32_t*>(g.cend));
  g.sorted = idx2;
  return hipGetLastError();
}

hipError_t launch_normals(const NbrGrid& g, float radius, const float vp[3], float4* out, hipStream_t s) {
  const int reach = std::max(1, (int)ceilf(radius * g.inv_cell));
  normals_kernel<<<grid_blocks(g.n), 256, 0, s>>>(g, radius * radius, reach, vp[0], vp[1], vp[2], out);
  return hipGetLastError();
}

hipError_t launch_rsd(const NbrGrid& g, const float4* nrm, const float4* cent, int64_t nc, float max_dist, float2* radii,
                      int32_t* types, hipStream_t s) {
  if (nc == 0) return hipSuccess;
  const int reach = std::max(1, (int)ceilf(max_dist * g.inv_cell));
  rsd_kernel<<<grid_blocks(nc), 256, 0, s>>>(g, nrm, cent, nc, max_dist, reach, radii, types);
  return hipGetLastError();
}

hipError_t launch_grsd(const GrsdArgs& a, hipStream_t s) {
  if (a.nc > 0) grsd_kernel<<<grid_blocks(a.nc), 256, 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_grsd_feat(const int32_t* trans, int64_t H, float norm, float* out, int stride, hipStream_t s) {
  if (H > 0) grsd_feat_kernel<<<grid_blocks(H * 20), 256, 0, s>>>(trans, H, norm, out, stride);
  return hipGetLastError();
}

hipError_t launch_vosch_concat(const float* grsd, const float* c3, const int32_t* exist, int64_t H, float* out,
                               hipStream_t s) {
  if (H > 0) vosch_concat_kernel<<<grid_blocks(H * 137), 256, 0, s>>>(grsd, c3, exist, H, out);
  return hipGetLastError();
}

}  // namespace c3h
