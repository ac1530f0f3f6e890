// c3_sparse.hip -- C3-HLAC-981 of a whole batch of frames from their sorted voxel lists, with no
// dense grid: columns 20 .. 1000 of the ConVOSCH rows of the batched voxel head (capi_vosch.hip).
//
// Every voxel is a centre at its acting cell a = floor(centroid / leaf) - min_b (voxs_moved's
// arithmetic), which gives its subdivision and the base of its 13 neighbours -- the semantics of
// offcell_contrib (c3hlac.hip), applied to every voxel instead of the few moved ones.  A
// neighbour is found by its own cell: a binary search of its linear index in the frame's
// ascending voxel keys, as vf_grsd_kernel finds its 26.
//
//   c3s_keys    thread = voxel of the batch: key = the batch ordinal of its row, or htot (none)
//   (rocPRIM)   one stable radix sort of (key, voxel ordinal): a row's voxels become consecutive
//   c3s_plan    thread = sorted position; a group's head finds the group's end, takes its chunks
//               (at most kC3sChunk voxels each) and, with several chunks, a slot of 64-bit sums
//   c3s_fill    zeros in columns 20 .. of every row of every good frame, a workgroup per row
//   c3s_accum   workgroup = chunk, per slice of kC3sSlice voxels two phases.  Stage: thread =
//               (voxel, position), its lookup, the centre or neighbour word unpacked to channel bytes
//               and beta bits into LDS (0 = absent).  Accumulate: thread = 4 of the 981 bins, each
//               a product of one field of the centre and one field of one staged position
//               (c3_sparse.h's table); the threads walk the staged voxels together, so every LDS
//               read is a broadcast of at most 14 neighbouring words, and sum in u32 registers.
//               No atomics and no same-address LDS writes: the order of summation cannot matter.
//               A group of one chunk writes (float)sum * norm981 into its row; others add their
//               sums to the group's 64-bit slot (integer adds: exact and order-free)
//   c3s_final   workgroup = group of several chunks: its slot into its row
//
// The numbers of groups and chunks stay on the device: the launches take the host's upper bounds
// (c3s_chunk_cap, c3s_multi_cap) and loop up to the device's counters.
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "c3_sparse.h"
#include "c3hlac_dev.h"

namespace c3h {
namespace {

__device__ const C3sTable kC3sTab = c3s_make_table();

int c3s_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

// the acting cell of a centroid, relative to the frame's min_b
__device__ __forceinline__ void c3s_acting(const GrsdArgs& ga, const float4& c, int a[3]) {
  a[0] = (int)floorf(__fdiv_rn(c.x, ga.leaf)) - ga.min_b[0];
  a[1] = (int)floorf(__fdiv_rn(c.y, ga.leaf)) - ga.min_b[1];
  a[2] = (int)floorf(__fdiv_rn(c.z, ga.leaf)) - ga.min_b[2];
}

__global__ __launch_bounds__(256) void c3s_keys_kernel(const VfTable* __restrict__ T, int64_t vtot, int64_t htot,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  for (int64_t q = blockIdx.x * (int64_t)256 + threadIdx.x; q < vtot; q += (int64_t)gridDim.x * 256) {
    const int f = vf_frame_of(T->vpre, T->nf, q);
    const GrsdArgs& ga = T->fr[f].ga;
    int a[3];
    c3s_acting(ga, ga.cent[q - T->vpre[f]], a);
    const int64_t h = c3s_subdivision(a, ga.off, ga.sb, ga.inv_s, ga.hist1);
    keys[q] = h < 0 || h >= T->hpre[f + 1] - T->hpre[f] ? c3s_none(htot) : c3s_key(T->hpre, f, h);
    idx[q] = (uint32_t)q;
  }
}

// cnt[0]: chunks, cnt[1]: groups of several chunks.  A workgroup plans a tile of kC3sPlanTile
// sorted positions and takes the chunk slots of all its heads with one atomic (a prefix sum over
// its threads): an atomic per wave, all on one address, was 0.45 ms of a 64-frame call.
constexpr int kC3sPlanItems = 8;
constexpr int kC3sPlanTile = 256 * kC3sPlanItems;
__global__ __launch_bounds__(256) void c3s_plan_kernel(const uint64_t* __restrict__ keys, int64_t vtot, int64_t htot,
                                                       int64_t chunk_cap, int64_t multi_cap, uint32_t* __restrict__ cnt,
                                                       C3sChunk* __restrict__ chunks, int64_t* __restrict__ multi_row) {
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = (vtot + kC3sPlanTile - 1) / kC3sPlanTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (uniform over the workgroup)
    int64_t len[kC3sPlanItems];
    uint32_t mine = 0;
#pragma unroll
    for (int it = 0; it < kC3sPlanItems; ++it) {
      const int64_t i = t * kC3sPlanTile + it * 256 + tid;
      int64_t L = 0;
      if (i < vtot) {
        const uint64_t k = keys[i];
        if (k < c3s_none(htot) && (i == 0 || keys[i - 1] != k)) {
          int64_t step = 1;  // groups are short: gallop to a position behind the group, then bisect
          while (i + step < vtot && keys[i + step] == k) step <<= 1;
          int64_t lo = i + (step >> 1) + 1, hi = i + step < vtot ? i + step : vtot;  // the first position whose key is larger
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] <= k) lo = mid + 1;
            else hi = mid;
          }
          L = lo - i;
        }
      }
      len[it] = L;
      mine += (uint32_t)c3s_chunks(L);
    }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (tid == 0) {
      const uint32_t tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
      s_base = tot ? atomicAdd(&cnt[0], tot) : 0u;
    }
    __syncthreads();
    int64_t base = (int64_t)s_base + incl - mine;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    __syncthreads();  // s_wave and s_base are read: the next tile may write them
#pragma unroll
    for (int it = 0; it < kC3sPlanItems; ++it) {
      const int64_t L = len[it], nch = c3s_chunks(L);
      if (nch == 0) continue;
      const int64_t i = t * kC3sPlanTile + it * 256 + tid;
      const uint64_t k = keys[i];
      int32_t multi = -1;
      bool ok = true;
      if (nch > 1) {
        const int64_t m = (int64_t)atomicAdd(&cnt[1], 1u);
        ok = m < multi_cap;  // (the bound of c3s_multi_cap: always)
        if (ok) {
          multi = (int32_t)m;
          multi_row[m] = (int64_t)k;
        }
      }
      for (int64_t c = 0; ok && c < nch && base + c < chunk_cap; ++c) {
        C3sChunk ch;
        ch.row = (int64_t)k;
        ch.start = (uint32_t)(i + c * kC3sChunk);
        ch.count = (uint32_t)c3s_chunk_len(L, c);
        ch.multi = multi;
        ch.pad = 0;
        chunks[base + c] = ch;
      }
      base += nch;
    }
  }
}

// a workgroup per row: 981 consecutive floats
__global__ __launch_bounds__(256) void c3s_fill_kernel(const VfTable* __restrict__ T, int64_t htot, int dim) {
  for (int64_t h = blockIdx.x; h < htot; h += gridDim.x) {
    const int f = vf_frame_of(T->hpre, T->nf, h);
    float* __restrict__ out = T->fr[f].rows + (h - T->hpre[f]) * dim + 20;
    const int w = dim - 20;
    const int head = (int)((16 - ((uintptr_t)out & 15)) & 15) >> 2;  // floats up to a 16-byte boundary (rows are 4-byte aligned)
    const int quads = head < w ? (w - head) >> 2 : 0;
    float4* __restrict__ body = reinterpret_cast<float4*>(out + head);
    for (int t = threadIdx.x; t < quads; t += 256) body[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int tail = head + 4 * quads;
    if ((int)threadIdx.x < head && (int)threadIdx.x < w) out[threadIdx.x] = 0.0f;
    if (tail + (int)threadIdx.x < w) out[tail + threadIdx.x] = 0.0f;
  }
}

// the staged word of a voxel word (24 colour bits)
__device__ __forceinline__ uint64_t c3s_stage_word(uint32_t word, const uint32_t* __restrict__ lut, const int thr[3]) {
  int a[6], be[6];
  channels(word, lut, thr, a, be);
  uint64_t w = (uint64_t)1 << 63;
#pragma unroll
  for (int c = 0; c < 6; ++c) w |= (uint64_t)(uint32_t)a[c] << (8 * c) | (uint64_t)(uint32_t)be[c] << (48 + c);
  return w;
}

struct C3sThr {
  int v[3];
};

__global__ __launch_bounds__(kC3sBlock) void c3s_accum_kernel(const VfTable* __restrict__ T,
                                                              const uint32_t* __restrict__ order,
                                                              const C3sChunk* __restrict__ chunks,
                                                              const uint32_t* __restrict__ cnt, int64_t chunk_cap,
                                                              const uint32_t* __restrict__ lut, C3sThr thr, int dim,
                                                              unsigned long long* __restrict__ acc) {
  __shared__ uint64_t s_w[kC3sSlice * kC3sPos];
  __shared__ uint32_t s_ex[2];
  const int tid = threadIdx.x;
  // this thread's bins: tid + kC3sBlock * i
  // (a field lies in one 32-bit half of a staged word: the position's half is read alone)
  int pos[kC3sBinsPerThread], sha[kC3sBinsPerThread], shb[kC3sBinsPerThread];
  uint32_t ma[kC3sBinsPerThread], mb[kC3sBinsPerThread];
  bool hia[kC3sBinsPerThread];
#pragma unroll
  for (int i = 0; i < kC3sBinsPerThread; ++i) {
    const uint32_t d = kC3sTab.v[tid + kC3sBlock * i];
    const int fa = (int)((d >> 4) & 63u), fb = (int)((d >> 10) & 63u);
    hia[i] = fa >= 32;
    sha[i] = fa & 31;
    pos[i] = 2 * (int)(d & 15u) + (fb >> 5);
    shb[i] = fb & 31;
    ma[i] = (d >> 18 & 1u) ? ((d >> 16 & 1u) ? 0xffu : 1u) : 0u;
    mb[i] = (d >> 18 & 1u) ? ((d >> 17 & 1u) ? 0xffu : 1u) : 0u;
  }
  const int64_t nchunks = std::min<int64_t>((int64_t)cnt[0], chunk_cap);
  for (int64_t ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const C3sChunk ch = chunks[ci];
    const int f = vf_frame_of(T->hpre, T->nf, ch.row);
    const VfFrame& fr = T->fr[f];
    const GrsdArgs& ga = fr.ga;
    const int32_t* __restrict__ vk = fr.vkeys;
    const int64_t nc = ga.nc, v0 = T->vpre[f];
    uint32_t sum[kC3sBinsPerThread];
#pragma unroll
    for (int i = 0; i < kC3sBinsPerThread; ++i) sum[i] = 0u;
    for (uint32_t s0 = 0; s0 < ch.count; s0 += kC3sSlice) {
      const int m = (int)std::min<uint32_t>(kC3sSlice, ch.count - s0);
      __syncthreads();  // the accumulate phase of the slice before has read s_w
      // stage: a (voxel, position) pair per thread and round, so that the lookups of a short
      // slice run side by side (a binary search is a chain of dependent loads)
      for (int e = tid; e < m * kC3sPos; e += kC3sBlock) {
        const int j = e / kC3sPos, p = e - j * kC3sPos;
        const int64_t v = (int64_t)order[ch.start + s0 + j] - v0;
        uint64_t w = 0;
        if (v >= 0 && v < nc) {  // (else a position of another frame: not reached)
          const float4 c = ga.cent[v];
          if (p == 0) {
            w = c3s_stage_word(__float_as_uint(c.w) & 0x00ffffffu, lut, thr.v);
          } else {
            int a[3], rel[3];
            c3s_acting(ga, c, a);
            c3s_rel(p - 1, rel);
            const int q0 = a[0] + rel[0], q1 = a[1] + rel[1], q2 = a[2] + rel[2];
            if (q0 >= 0 && q0 < ga.div_b[0] && q1 >= 0 && q1 < ga.div_b[1] && q2 >= 0 && q2 < ga.div_b[2]) {
              const int64_t lin = q0 + (int64_t)ga.div_b[0] * (q1 + (int64_t)ga.div_b[1] * q2);
              // the first key >= lin.  The keys ascend and differ, so from v's own key the position
              // lies no further off than the keys do
              const int64_t own = vk[v], off = lin - own;
              int64_t lo = off < 0 ? (v + off > 0 ? v + off : 0) : v, hi = off < 0 ? v : (v + off + 1 < nc ? v + off + 1 : nc);
              while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (vk[mid] < lin) lo = mid + 1;
                else hi = mid;
              }
              if (lo < nc && vk[lo] == lin) w = c3s_stage_word(__float_as_uint(ga.cent[lo].w) & 0x00ffffffu, lut, thr.v);
            }
          }
        }
        s_w[e] = w;
      }
      __syncthreads();
      for (int j = 0; j < m; ++j) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(s_w + j * kC3sPos);
        const uint32_t clo = w[0], chi = w[1];
#pragma unroll
        for (int i = 0; i < kC3sBinsPerThread; ++i)
          sum[i] += (((hia[i] ? chi : clo) >> sha[i]) & ma[i]) * ((w[pos[i]] >> shb[i]) & mb[i]);
      }
    }
    if (ch.multi >= 0) {
      unsigned long long* slot = acc + (int64_t)ch.multi * kC3sBins;
#pragma unroll
      for (int i = 0; i < kC3sBinsPerThread; ++i) {
        const int bin = tid + kC3sBlock * i;
        if (bin < kC3sBins && sum[i]) atomicAdd(&slot[bin], (unsigned long long)sum[i]);
      }
    } else {
      __syncthreads();  // s_ex of the chunk before is read
      if (tid < 2) s_ex[tid] = sum[0];
      __syncthreads();
      const bool ex = exist_from((float)s_ex[0], (float)s_ex[1]) != 0;
      float* out = fr.rows + (ch.row - T->hpre[f]) * dim + 20;
#pragma unroll
      for (int i = 0; i < kC3sBinsPerThread; ++i) {
        const int bin = tid + kC3sBlock * i;
        if (bin < kC3sBins) out[bin] = ex ? (float)sum[i] * norm981(bin) : 0.0f;
      }
    }
  }
}

__global__ __launch_bounds__(256) void c3s_final_kernel(const VfTable* __restrict__ T, const uint32_t* __restrict__ cnt,
                                                        int64_t multi_cap, const int64_t* __restrict__ multi_row,
                                                        const unsigned long long* __restrict__ acc, int dim) {
  const int64_t nm = std::min<int64_t>((int64_t)cnt[1], multi_cap);
  for (int64_t m = blockIdx.x; m < nm; m += gridDim.x) {
    const unsigned long long* hist = acc + m * kC3sBins;
    const int64_t row = multi_row[m];
    const int f = vf_frame_of(T->hpre, T->nf, row);
    float* out = T->fr[f].rows + (row - T->hpre[f]) * dim + 20;
    const bool ex = exist_from((float)hist[0], (float)hist[1]) != 0;
    for (int i = threadIdx.x; i < kC3sBins; i += 256) out[i] = ex ? (float)hist[i] * norm981(i) : 0.0f;
  }
}

}  // namespace

hipError_t launch_c3_sparse(const VfTable* d_tab, int64_t vtot, int64_t htot, const C3sBufs& b, const uint32_t* lut,
                            const int32_t thr[3], int dim, hipStream_t s) {
  const size_t n = (size_t)std::max<int64_t>(vtot, 1);
  const int bits = c3s_key_bits(htot);
  if (!b.tmp) {  // size query
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, b.keys, b.keys2, b.idx, b.idx2, n, 0, bits, s);
    *b.tmp_bytes = bytes;
    return e;
  }
  if (htot <= 0) return hipSuccess;
  c3s_fill_kernel<<<(int)std::min<int64_t>(htot, 16384), 256, 0, s>>>(d_tab, htot, dim);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || vtot <= 0) return e;
  const int64_t chunk_cap = c3s_chunk_cap(vtot, htot), multi_cap = c3s_multi_cap(vtot);
  e = hipMemsetAsync(b.cnt, 0, 2 * sizeof(uint32_t), s);
  if (e == hipSuccess && multi_cap > 0) e = hipMemsetAsync(b.acc, 0, (size_t)multi_cap * kC3sBins * 8, s);
  if (e != hipSuccess) return e;
  c3s_keys_kernel<<<c3s_blocks(vtot), 256, 0, s>>>(d_tab, vtot, htot, b.keys, b.idx);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = *b.tmp_bytes;
  e = rocprim::radix_sort_pairs(b.tmp, bytes, b.keys, b.keys2, b.idx, b.idx2, (size_t)vtot, 0, bits, s);
  if (e != hipSuccess) return e;
  c3s_plan_kernel<<<(int)std::min<int64_t>((vtot + kC3sPlanTile - 1) / kC3sPlanTile, 8192), 256, 0, s>>>(b.keys2, vtot, htot, chunk_cap, multi_cap, b.cnt, b.chunks, b.multi_row);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  C3sThr t;
  for (int a = 0; a < 3; ++a) t.v[a] = thr[a];
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(chunk_cap, 4096));
  c3s_accum_kernel<<<blocks, kC3sBlock, 0, s>>>(d_tab, b.idx2, b.chunks, b.cnt, chunk_cap, lut, t, dim, b.acc);
  e = hipGetLastError();
  if (e != hipSuccess || multi_cap == 0) return e;
  c3s_final_kernel<<<(int)std::min<int64_t>(multi_cap, 4096), 256, 0, s>>>(d_tab, b.cnt, multi_cap, b.multi_row, b.acc, dim);
  return hipGetLastError();
}

}  // namespace c3h
