// vosch_front.hip -- normals, RSD radii, GRSD transition histograms and feature rows on the GPU
// (the VOSCH / GRSD features of color_chlac/include/color_chlac/
// grsd_colorCHLAC_tools.hpp:63-296, 832-843) for every frame of a batch in one set of launches;
// a single frame (c3h_compute_normals, c3h_extract_grsd / c3h_extract_vosch) is a batch of one.
// The arithmetic is in rsd_dev.h.
//
// Radius searches run over a dense grid of cells of the normal radius: the points are sorted by
// cell (rocPRIM radix sort of (cell, point) pairs: stable, so a cell lists its points in input
// order) and every cell keeps its [start, end) range.  A query visits the cells within
// ceil(radius / cell) of its own.
//   normals: double sums of the neighbours within the radius (the point included, squared
//     distances in float as FLANN compares them); covariance -> smallest-eigenvalue eigenvector
//     (Jacobi, double), flipped towards the viewpoint, curvature = lambda_min / trace;
//     < 3 neighbours -> NaN (PCL).  A point the voxeliser dropped is nobody's neighbour and gets NaN.
//   RSD: one downsampled centroid per thread; PCL's computeRSD over the cloud points within
//     max(rsd_radius, leaf sqrt(3) / 2) of it: the nearest one is the reference ("begin"), the
//     others' normal angles are binned by their distance to it.
//   GRSD: one occupied voxel per thread; its type against the 26 neighbour voxels (EMPTY where
//     unoccupied), int atomics into its subdivision's 6 x 6 matrix.
//
// The frames' points are concatenated by a prefix of their counts.  One keys kernel files every
// point under the composite key (frame << cell_bits | cell) of its frame's own search grid, one
// stable rocPRIM radix sort orders them -- per frame: cell order, then input order --, one
// ranges kernel writes the frames' concatenated cell tables.
//   vf_dense_list_kernel lists the cells of kVfDenseCell points and more;
//   vf_normals_kernel: the work unit is such a cell, not a point.  One wave takes a cell:
//     the points of the (2 reach + 1)^3 cells around it are staged in LDS in chunks of kVfChunk,
//     in the visiting order of for_neighbours (dz, dy, dx ascending, then sorted order); each
//     lane owns one query of the cell and walks the staged points with broadcast LDS reads.  A
//     neighbour is read from global memory once per 64 queries instead of once per pair.  The
//     distance test, the ten double sums and the eigen solve are the per-point walk's functions,
//     the sums are added in the same order: the normals are the per-point walk's bit for bit.
//     Cells of fewer than kVfDenseCell points are left to
//   vf_normals_sparse_kernel: one sorted position per thread with the per-pair walk
//     (a wave that stages 27 cells for two or three queries idles its lanes), and the points in
//     no cell (the voxeliser dropped them: NaN).
//   vf_normals_frame_kernel: a table of one frame, one point per thread with the per-pair walk.
//     The dense cells of one frame are too few waves to fill the device, and the densest of them
//     is a tail that only a batch hides.
//   vf_rsd_kernel / vf_grsd_kernel: one centroid per thread over all frames on the frame's table
//     record.  A neighbour voxel's type is found by a binary search
//     of its linear index in the frame's sorted voxel keys (a few KB per frame, against a layout
//     grid of div_b product words per frame that a batch would have to keep 64 of); a single
//     frame still has its leaf layout and looks the voxel up there.
//   vf_rows_kernel: columns 0 .. 19 of every row of every frame.
#include <rocprim/device/device_radix_sort.hpp>

#include "c3h_internal.h"
#include "rsd_dev.h"

namespace c3h {
namespace {

constexpr int kVfChunk = 256;  // staged points per pass: 4 KB of LDS per one-wave workgroup
// Cells of fewer points go to the per-point kernel: a wave that stages a neighbourhood for a
// handful of queries idles most of its lanes (measured on sparse Kinect scenes)
constexpr int kVfDenseCell = 16;
static_assert(kVfDenseCell == kVfDenseMin, "the dense-cell list is sized by kVfDenseMin");
constexpr int kVfNbMax = (2 * kVfMaxReach + 1) * (2 * kVfMaxReach + 1) * (2 * kVfMaxReach + 1);

int grid_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

template <class K>
__global__ void vf_keys_kernel(const VfTable* __restrict__ T, int which, int cell_bits, int64_t ptot,
                               K* __restrict__ keys, uint32_t* __restrict__ idx) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ptot; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = vf_frame_of(T->ppre, T->nf, i);
    const int64_t li = i - T->ppre[f];
    const NbrGrid& g = which ? T->fr[f].g2 : T->fr[f].g;
    const float4 p = g.pts[li];
    int c[3];
    const uint64_t cell = pt_kept(g, p) && cell_of(g, p, c) ? (uint64_t)(c[0] + g.dim[0] * (c[1] + g.dim[1] * c[2]))
                                                            : vf_no_cell(cell_bits);
    keys[i] = (K)vf_make_key(f, cell, cell_bits);
    idx[i] = (uint32_t)li;
  }
}

// cstart / cend: the concatenated tables; the values are positions in the frame's own slice
template <class K>
__global__ void vf_ranges_kernel(const VfTable* __restrict__ T, int which, int cell_bits, int64_t ptot,
                                 const K* __restrict__ keys, uint32_t* __restrict__ cstart,
                                 uint32_t* __restrict__ cend) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ptot; i += (int64_t)gridDim.x * blockDim.x) {
    const K k = keys[i];
    const uint64_t cell = vf_key_cell(k, cell_bits);
    if (cell == vf_no_cell(cell_bits)) continue;
    const int f = vf_key_frame(k, cell_bits);
    if (f < 0 || f >= T->nf) continue;
    const int64_t c0 = which ? T->c2pre[f] : T->cpre[f];
    const int64_t c1 = which ? T->c2pre[f + 1] : T->cpre[f + 1];
    if ((int64_t)cell >= c1 - c0) continue;
    const int64_t p0 = T->ppre[f];
    if (i == 0 || keys[i - 1] != k) cstart[c0 + cell] = (uint32_t)(i - p0);
    if (i == ptot - 1 || keys[i + 1] != k) cend[c0 + cell] = (uint32_t)(i + 1 - p0);
  }
}

// The dense cells of all frames (concatenated cell index), in no particular order: every cell is
// a work item of its own, so a row of dense cells along a wall spreads over the device instead of
// queueing in the one wave that scans it.  list[0] is the counter (zeroed before the launch).
__global__ void vf_dense_list_kernel(const VfTable* __restrict__ T, int64_t ctot, int64_t cap,
                                     unsigned long long* __restrict__ list) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < ctot; c += (int64_t)gridDim.x * blockDim.x) {
    const int f = vf_frame_of(T->cpre, T->nf, c);
    const NbrGrid& g = T->fr[f].g;
    const int64_t cell = c - T->cpre[f];
    if (g.cend[cell] - g.cstart[cell] >= (uint32_t)kVfDenseCell) {
      const unsigned long long at = atomicAdd(&list[0], 1ull);
      if ((int64_t)at < cap) list[1 + at] = (unsigned long long)c;
    }
  }
}

// One wave per workgroup; every loop bound below is the same in all its lanes.
__global__ __launch_bounds__(64) void vf_normals_kernel(const VfTable* __restrict__ T, int64_t cap,
                                                        const unsigned long long* __restrict__ list, float r2, int reach,
                                                        float vx, float vy, float vz, float4* __restrict__ out) {
  __shared__ float4 sp[kVfChunk];
  __shared__ uint32_t s_start[kVfNbMax];
  __shared__ uint32_t s_pre[kVfNbMax + 1];
  const int lane = threadIdx.x;
  const int w = 2 * reach + 1, nn = w * w * w;
  const int64_t nitems = (int64_t)list[0] < cap ? (int64_t)list[0] : cap;
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    {
      const int64_t gc = (int64_t)list[1 + item];
      const int f = vf_frame_of(T->cpre, T->nf, gc);
      const NbrGrid& g = T->fr[f].g;
      const int64_t p0 = T->ppre[f];
      const int cell = (int)(gc - T->cpre[f]);
      const int cx = cell % g.dim[0], cy = (cell / g.dim[0]) % g.dim[1], cz = cell / (g.dim[0] * g.dim[1]);
      __syncthreads();  // the previous cell's tables and stage are read out
      for (int t = lane; t < nn; t += 64) {  // the ranges of the cells around, in visiting order
        const int x = cx + t % w - reach, y = cy + (t / w) % w - reach, z = cz + t / (w * w) - reach;
        uint32_t s0 = 0, len = 0;
        if (x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2]) {
          const int nc = x + g.dim[0] * (y + g.dim[1] * z);
          s0 = g.cstart[nc];
          const uint32_t e = g.cend[nc];
          len = e > s0 ? e - s0 : 0;
        }
        s_start[t] = s0;
        s_pre[t + 1] = len;
      }
      __syncthreads();
      if (lane == 0) {
        uint32_t acc = 0;
        s_pre[0] = 0;
        for (int t = 0; t < nn; ++t) {
          acc += s_pre[t + 1];
          s_pre[t + 1] = acc;
        }
      }
      __syncthreads();
      const uint32_t total = s_pre[nn];
      const uint32_t qs = g.cstart[cell], qe = g.cend[cell];
      for (uint32_t qb = qs; qb < qe; qb += 64) {
        const bool mine = qb + lane < qe;
        const uint32_t j = mine ? g.sorted[qb + lane] : 0;
        const float4 q = mine ? g.pts[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t c0 = 0; c0 < total; c0 += kVfChunk) {
          const uint32_t cnt = total - c0 < (uint32_t)kVfChunk ? total - c0 : (uint32_t)kVfChunk;
          __syncthreads();  // the previous chunk is consumed
          for (uint32_t e = lane; e < cnt; e += 64) {
            const uint32_t t = c0 + e;
            int lo = 0, hi = nn;  // the cell range holding staged element t: s_pre[lo] <= t < s_pre[hi]
            while (hi - lo > 1) {
              const int mid = (lo + hi) >> 1;
              if (s_pre[mid] <= t) lo = mid;
              else hi = mid;
            }
            sp[e] = g.pts[g.sorted[s_start[lo] + (t - s_pre[lo])]];
          }
          __syncthreads();
          if (mine) {
            uint32_t e = 0;
            for (; e + 4 <= cnt; e += 4) {  // four LDS reads in flight; the sums keep their order
              const float4 pa = sp[e], pb = sp[e + 1], pc = sp[e + 2], pd = sp[e + 3];
              if (pair_d2(pa, q) < r2) nrm_accum(s, pa);
              if (pair_d2(pb, q) < r2) nrm_accum(s, pb);
              if (pair_d2(pc, q) < r2) nrm_accum(s, pc);
              if (pair_d2(pd, q) < r2) nrm_accum(s, pd);
            }
            for (; e < cnt; ++e) {
              const float4 p = sp[e];
              if (pair_d2(p, q) < r2) nrm_accum(s, p);
            }
          }
        }
        if (mine) out[p0 + j] = nrm_from_sums(s, q, vx, vy, vz);
      }
    }
  }
}

// The queries of the cells below kVfDenseCell points, and the points in no cell: one sorted
// position per thread, the per-pair walk (neighbouring threads are neighbouring points).  A dropped point (non-finite, z >= z_limit) gets NaN.
template <class K>
__global__ void vf_normals_sparse_kernel(const VfTable* __restrict__ T, int cell_bits, int64_t ptot,
                                         const K* __restrict__ sorted_keys, float r2, int reach, float vx, float vy,
                                         float vz, float4* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ptot; i += (int64_t)gridDim.x * blockDim.x) {
    const K k = sorted_keys[i];
    const int f = vf_key_frame(k, cell_bits);
    if (f < 0 || f >= T->nf) continue;
    const NbrGrid& g = T->fr[f].g;
    const uint64_t cell = vf_key_cell(k, cell_bits);
    if (cell != vf_no_cell(cell_bits) && (int64_t)cell < T->cpre[f + 1] - T->cpre[f] &&
        g.cend[cell] - g.cstart[cell] >= (uint32_t)kVfDenseCell)
      continue;  // a query of the cell-staged kernel
    const int64_t p0 = T->ppre[f];
    const uint32_t j = g.sorted[i - p0];
    out[p0 + j] = nrm_point(g, g.pts[j], r2, reach, vx, vy, vz);
  }
}

// every point of a one-frame table by the per-pair walk, in input order
__global__ void vf_normals_frame_kernel(const VfTable* __restrict__ T, float r2, int reach, float vx, float vy, float vz,
                                        float4* __restrict__ out) {
  const NbrGrid& g = T->fr[0].g;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = nrm_point(g, g.pts[i], r2, reach, vx, vy, vz);
}

__global__ void vf_rsd_kernel(const VfTable* __restrict__ T, int64_t vtot, const float4* __restrict__ nrm,
                              float max_dist, int reach, float2* __restrict__ radii, int32_t* __restrict__ types) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < vtot; c += (int64_t)gridDim.x * blockDim.x) {
    const int f = vf_frame_of(T->vpre, T->nf, c);
    const VfFrame& fr = T->fr[f];
    rsd_point(fr.g2, nrm + T->ppre[f], fr.ga.cent[c - T->vpre[f]], max_dist, reach, &radii[c], &types[c]);
  }
}

__global__ void vf_grsd_kernel(const VfTable* __restrict__ T, int64_t vtot) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < vtot; c += (int64_t)gridDim.x * blockDim.x) {
    const int f = vf_frame_of(T->vpre, T->nf, c);
    const VfFrame& fr = T->fr[f];
    const int32_t* vk = fr.vkeys;
    const int32_t* layout = fr.layout;
    const int64_t nc = fr.ga.nc;
    grsd_voxel(fr.ga, c - T->vpre[f], [&](int64_t v) {
      if (layout) return layout[v];
      int64_t lo = 0, hi = nc;  // the first key >= v
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (vk[mid] < v) lo = mid + 1;
        else hi = mid;
      }
      return lo < nc && vk[lo] == v ? (int32_t)lo : -1;
    });
  }
}

// upper-triangle bins of each frame's 6 x 6 matrices into columns 0 .. 19 of its rows, times norm
__global__ void vf_rows_kernel(const VfTable* __restrict__ T, int64_t htot, const int32_t* __restrict__ trans,
                               float norm, int dim) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < htot * 20; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t h = e / 20;
    const int b = (int)(e - h * 20);
    const int f = vf_frame_of(T->hpre, T->nf, h);
    T->fr[f].rows[(h - T->hpre[f]) * dim + b] = (float)trans[h * 36 + grsd_bin_cell(b)] * norm;
  }
}

__global__ void vf_vox_keys_kernel(const int32_t* __restrict__ layout, int64_t nvox, int64_t nc,
                                   int32_t* __restrict__ vkeys) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    const int32_t li = layout[v];
    if (li >= 0 && li < nc) vkeys[li] = (int32_t)v;
  }
}

// columns 20 .. of a frame's VOSCH (117 of 137) or ConVOSCH (981 of 1001) rows: its C3-HLAC rows,
// zeros where exist is 0 (rows of empty subdivisions may be stale)
__global__ void vf_c3_cols_kernel(const float* __restrict__ c3, const int32_t* __restrict__ exist, int64_t H,
                                  int variant, int stride, float* __restrict__ rows) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < H * variant; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t h = e / variant;
    const int t = (int)(e - h * variant);
    rows[h * stride + 20 + t] = exist[h] ? c3[e] : 0.0f;
  }
}

template <class K>
hipError_t nbr_build_t(const VfTable* d_tab, int which, const VfKey& key, int64_t ptot, int64_t ctot, K* keys, K* keys2,
                       uint32_t* idx, uint32_t* idx2, uint32_t* cstart, uint32_t* cend, void* tmp, size_t* tmp_bytes,
                       hipStream_t s) {
  if (!tmp) {  // size query
    size_t b = 0;
    const hipError_t e =
        rocprim::radix_sort_pairs(nullptr, b, keys, keys2, idx, idx2, (size_t)std::max<int64_t>(ptot, 1), 0, key.bits, s);
    *tmp_bytes = b;
    return e;
  }
  hipError_t e = hipMemsetAsync(cstart, 0, (size_t)std::max<int64_t>(ctot, 1) * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(cend, 0, (size_t)std::max<int64_t>(ctot, 1) * 4, s);
  if (e != hipSuccess || ptot == 0) return e;
  vf_keys_kernel<K><<<grid_blocks(ptot), 256, 0, s>>>(d_tab, which, key.cell_bits, ptot, keys, idx);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t b = *tmp_bytes;
  e = rocprim::radix_sort_pairs(tmp, b, keys, keys2, idx, idx2, (size_t)ptot, 0, key.bits, s);
  if (e != hipSuccess) return e;
  vf_ranges_kernel<K><<<grid_blocks(ptot), 256, 0, s>>>(d_tab, which, key.cell_bits, ptot, keys2, cstart, cend);
  return hipGetLastError();
}

}  // namespace

hipError_t vf_nbr_build(const VfTable* d_tab, int which, const VfKey& key, int64_t ptot, int64_t ctot, void* keys,
                        void* keys2, uint32_t* idx, uint32_t* idx2, uint32_t* cstart, uint32_t* cend, void* tmp,
                        size_t* tmp_bytes, hipStream_t s) {
  if (key.wide)
    return nbr_build_t<uint64_t>(d_tab, which, key, ptot, ctot, (uint64_t*)keys, (uint64_t*)keys2, idx, idx2, cstart, cend,
                                 tmp, tmp_bytes, s);
  return nbr_build_t<uint32_t>(d_tab, which, key, ptot, ctot, (uint32_t*)keys, (uint32_t*)keys2, idx, idx2, cstart, cend,
                               tmp, tmp_bytes, s);
}

hipError_t launch_vf_normals(const VfTable* d_tab, int nf, const VfKey& key, int64_t ptot, int64_t ctot, const void* keys,
                             unsigned long long* list, float radius, int reach, const float vp[3], float4* out,
                             hipStream_t s) {
  if (reach < 1 || reach > kVfMaxReach) return hipErrorInvalidValue;
  if (ptot == 0) return hipSuccess;
  const float r2 = radius * radius;
  if (nf == 1) {
    vf_normals_frame_kernel<<<grid_blocks(ptot), 256, 0, s>>>(d_tab, r2, reach, vp[0], vp[1], vp[2], out);
    return hipGetLastError();
  }
  if (ctot > 0) {
    const int64_t cap = vf_dense_cap(ptot);
    hipError_t e = hipMemsetAsync(list, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    vf_dense_list_kernel<<<grid_blocks(ctot), 256, 0, s>>>(d_tab, ctot, cap, list);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cap, 65536));
    vf_normals_kernel<<<blocks, 64, 0, s>>>(d_tab, cap, list, r2, reach, vp[0], vp[1], vp[2], out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (key.wide)
    vf_normals_sparse_kernel<uint64_t><<<grid_blocks(ptot), 256, 0, s>>>(d_tab, key.cell_bits, ptot, (const uint64_t*)keys,
                                                                        r2, reach, vp[0], vp[1], vp[2], out);
  else
    vf_normals_sparse_kernel<uint32_t><<<grid_blocks(ptot), 256, 0, s>>>(d_tab, key.cell_bits, ptot, (const uint32_t*)keys,
                                                                        r2, reach, vp[0], vp[1], vp[2], out);
  return hipGetLastError();
}

hipError_t launch_vf_rsd(const VfTable* d_tab, int64_t vtot, const float4* nrm, float max_dist, int reach,
                         float2* radii, int32_t* types, hipStream_t s) {
  if (vtot > 0) vf_rsd_kernel<<<grid_blocks(vtot), 256, 0, s>>>(d_tab, vtot, nrm, max_dist, reach, radii, types);
  return hipGetLastError();
}

hipError_t launch_vf_grsd(const VfTable* d_tab, int64_t vtot, hipStream_t s) {
  if (vtot > 0) vf_grsd_kernel<<<grid_blocks(vtot), 256, 0, s>>>(d_tab, vtot);
  return hipGetLastError();
}

hipError_t launch_vf_rows(const VfTable* d_tab, int64_t htot, const int32_t* trans, float norm, int dim, hipStream_t s) {
  if (htot > 0) vf_rows_kernel<<<grid_blocks(htot * 20), 256, 0, s>>>(d_tab, htot, trans, norm, dim);
  return hipGetLastError();
}

hipError_t launch_vf_vox_keys(const int32_t* layout, int64_t nvox, int64_t nc, int32_t* vkeys, hipStream_t s) {
  if (nvox > 0 && nc > 0) vf_vox_keys_kernel<<<grid_blocks(nvox), 256, 0, s>>>(layout, nvox, nc, vkeys);
  return hipGetLastError();
}

hipError_t launch_vf_c3_cols(const float* c3, const int32_t* exist, int64_t H, int variant, int stride, float* rows,
                             hipStream_t s) {
  if (H > 0) vf_c3_cols_kernel<<<grid_blocks(H * variant), 256, 0, s>>>(c3, exist, H, variant, stride, rows);
  return hipGetLastError();
}

}  // namespace c3h
