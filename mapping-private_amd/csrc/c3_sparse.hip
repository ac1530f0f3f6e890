// c3_sparse.hip -- C3-HLAC-981 / 117 of a whole batch of frames from their sorted voxel lists, with
// no dense grid: columns 20 .. 1000 of the ConVOSCH rows of the batched voxel head, and the rows and
// exist values of c3h_extract_c3_frames at either variant (capi_vosch.hip).
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
//   c3s_fill    zeros in the columns of every row of every good frame, a workgroup (117: a wave) per row
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
//   c3s117_accum  variant 117 in place of c3s_accum: wave = chunk; the 13 neighbours of a voxel are
//               summed per field before the products (its own comment, below)
//
// The numbers of groups and chunks stay on the device: the launches take the host's upper bounds
// (c3s_chunk_cap, c3s_multi_cap) and loop up to the device's counters.
//
// Packed mode (c3h_extract_c3_frames_packed, c3h_pca_add_c3_frames; launch_c3_packed): only the rows
// that hold a voxel are written, one after another in the order of the sorted keys.  No fill.
//   c3s_pack_count   workgroup = plan tile: its group heads
//   c3s_pack_scan    one workgroup: the exclusive scan of the tiles' heads
//   c3s_pack_frames  workgroup = frame: the heads in front of its first key (the host reads them)
//   c3s_plan<true>   a head's packed position from the scan and its tile's ballots, into its chunks
//                    (and multi_slot), -1 past the caller's capacity; frame and row of its id record
//   c3s_accum<true>, c3s117_accum<true>, c3s_final<., true>  skip what has no slot; the epilogues
//                    write rows + slot * variant and the id record's exist value
// Every step is a launch boundary: no workgroup waits on another, no ordinal is an atomic's return.
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "c3_sparse.h"
#include "c3hlac_dev.h"

namespace c3h {
namespace {

__device__ const C3sTable kC3sTab = c3s_make_table();
__device__ const C3s117Table kC3s117Tab = c3s117_make_table();

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
// kPacked: every head also takes its packed position (c3_sparse.h: the tiles before from
// tile_base, the heads before within the tile from the waves' ballots), which its chunks and, with
// several chunks, multi_slot carry, or -1 where the position lies at or past pack_cap; the frame
// and row of its id record are written here.
template <bool kPacked>
__global__ __launch_bounds__(256) void c3s_plan_kernel(const uint64_t* __restrict__ keys, int64_t vtot, int64_t htot,
                                                       int64_t chunk_cap, int64_t multi_cap, uint32_t* __restrict__ cnt,
                                                       C3sChunk* __restrict__ chunks, int64_t* __restrict__ multi_row,
                                                       const int64_t* __restrict__ tile_base, int64_t pack_base,
                                                       int64_t* __restrict__ multi_slot, const VfTable* __restrict__ T,
                                                       C3sPackedRow* __restrict__ ids, int64_t pack_cap, int frame0) {
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_base;
  __shared__ uint32_t s_heads[kPacked ? kC3sPlanItems * kC3sPlanWaves : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = (vtot + kC3sPlanTile - 1) / kC3sPlanTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (uniform over the workgroup)
    int64_t len[kC3sPlanItems];
    uint64_t bal[kPacked ? kC3sPlanItems : 1];
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
      if constexpr (kPacked) {
        bal[it] = __ballot(L > 0);
        if (lane == 0) s_heads[it * kC3sPlanWaves + wave] = (uint32_t)__popcll(bal[it]);
      }
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
      int64_t slot = -1;
      if constexpr (kPacked) {
        slot = c3s_pack_slot(pack_base, tile_base[t], c3s_pack_local(s_heads, it, wave, bal[it], lane));
        if (!c3s_slot_written(slot, pack_cap)) {
          slot = -1;  // past the caller's capacity: its chunks are skipped, nothing of it is written
        } else if (ids) {  // (the row's exist value: the epilogue that sums it)
          const int f = vf_frame_of(T->hpre, T->nf, (int64_t)k);
          ids[slot].frame = frame0 + f;
          ids[slot].row = (int64_t)k - T->hpre[f];
        }
      }
      int32_t multi = -1;
      bool ok = true;
      if (nch > 1) {
        const int64_t m = (int64_t)atomicAdd(&cnt[1], 1u);
        ok = m < multi_cap;  // (the bound of c3s_multi_cap: always)
        if (ok) {
          multi = (int32_t)m;
          multi_row[m] = (int64_t)k;
          if constexpr (kPacked) multi_slot[m] = slot;
        }
      }
      for (int64_t c = 0; ok && c < nch && base + c < chunk_cap; ++c) {
        C3sChunk ch;
        ch.row = (int64_t)k;
        ch.start = (uint32_t)(i + c * kC3sChunk);
        ch.count = (uint32_t)c3s_chunk_len(L, c);
        ch.multi = multi;
        ch.pad = 0;
        ch.slot = slot;
        chunks[base + c] = ch;
      }
      base += nch;
    }
    if constexpr (kPacked) __syncthreads();  // s_heads is read: the next tile writes it
  }
}

// ---- the packed position of a group (c3_sparse.h) ----------------------------------------------------
// the heads of every plan tile
__global__ __launch_bounds__(256) void c3s_pack_count_kernel(const uint64_t* __restrict__ keys, int64_t vtot, int64_t htot,
                                                             uint32_t* __restrict__ tile_heads) {
  __shared__ uint32_t s_n[kC3sPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntiles = c3s_plan_tiles(vtot);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (uniform over the workgroup)
    uint32_t n = 0;
#pragma unroll
    for (int it = 0; it < kC3sPlanItems; ++it) {
      const int64_t i = c3s_plan_pos(t, it, tid);
      n += (uint32_t)__popcll(__ballot(i < vtot && c3s_head(keys, i, c3s_none(htot))));
    }
    if (lane == 0) s_n[wave] = n;
    __syncthreads();
    if (tid == 0) tile_heads[t] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    __syncthreads();  // s_n is read: the next tile writes it
  }
}

// One workgroup: tile_base[t] = the heads of the tiles before t, tile_base[ntiles] their number.  The
// tiles go 256 at a time, the carry in a register of every thread.
__global__ __launch_bounds__(256) void c3s_pack_scan_kernel(const uint32_t* __restrict__ tile_heads, int64_t ntiles,
                                                            int64_t* __restrict__ tile_base) {
  __shared__ uint32_t s_wave[kC3sPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < ntiles; b0 += 256) {
    const int64_t i = b0 + tid;
    const uint32_t v = i < ntiles ? tile_heads[i] : 0u;
    uint32_t incl = v;  // (a round holds at most 256 * kC3sPlanTile heads)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t pre = 0;
    for (int w = 0; w < wave; ++w) pre += s_wave[w];
    if (i < ntiles) tile_base[i] = carry + pre + incl - v;
    carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();  // s_wave is read: the next round writes it
  }
  if (tid == 0) tile_base[ntiles] = carry;
}

// Workgroup f = 0 .. nf: frame_first[f] = the heads in front of frame f's first key, i.e. in front of
// the first sorted position whose key is hpre[f] or more (hpre[nf] = htot, the "none" key: all heads)
__global__ __launch_bounds__(256) void c3s_pack_frames_kernel(const VfTable* __restrict__ T, const uint64_t* __restrict__ keys,
                                                              int64_t vtot, const int64_t* __restrict__ tile_base,
                                                              int64_t* __restrict__ frame_first) {
  __shared__ uint32_t s_n[kC3sPlanWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.x;
  const uint64_t key = (uint64_t)T->hpre[f], none = c3s_none(T->hpre[T->nf]);
  int64_t lo = 0, hi = vtot;  // (the same search in every thread)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  const int64_t t = lo / kC3sPlanTile;
  uint32_t n = 0;
#pragma unroll
  for (int it = 0; it < kC3sPlanItems; ++it) {
    const int64_t i = c3s_plan_pos(t, it, tid);
    n += (uint32_t)__popcll(__ballot(i < lo && c3s_head(keys, i, none)));
  }
  if (lane == 0) s_n[wave] = n;
  __syncthreads();
  if (tid == 0) frame_first[f] = tile_base[t] + (s_n[0] + s_n[1] + s_n[2] + s_n[3]);  // (lo == vtot on a tile's edge: t = ntiles, no head counted)
}

// kPer rows per workgroup, 256 / kPer threads each (1: a workgroup per row of 981; 4: a wave per
// row of 117, whose 30 quads leave most of a workgroup idle): w consecutive floats from column
// col0, and the row's exist value
template <int kPer>
__global__ __launch_bounds__(256) void c3s_fill_kernel(const VfTable* __restrict__ T, int64_t htot, int w, int stride,
                                                       int col0) {
  constexpr int kN = 256 / kPer;
  const int t = kPer == 1 ? (int)threadIdx.x : (int)threadIdx.x % kN;
  const int sub = kPer == 1 ? 0 : (int)threadIdx.x / kN;  // (1: the row stays uniform over the workgroup, in scalar registers)
  for (int64_t h = (int64_t)blockIdx.x * kPer + sub; h < htot; h += (int64_t)gridDim.x * kPer) {
    const int f = vf_frame_of(T->hpre, T->nf, h);
    float* __restrict__ out = T->fr[f].rows + (h - T->hpre[f]) * stride + col0;
    if (t == 0 && T->fr[f].exist) T->fr[f].exist[h - T->hpre[f]] = 0;
    const int head = (int)((16 - ((uintptr_t)out & 15)) & 15) >> 2;  // floats up to a 16-byte boundary (rows are 4-byte aligned)
    const int quads = head < w ? (w - head) >> 2 : 0;
    float4* __restrict__ body = reinterpret_cast<float4*>(out + head);
    for (int q = t; q < quads; q += kN) body[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int tail = head + 4 * quads;
    if (t < head && t < w) out[t] = 0.0f;
    if (tail + t < w) out[tail + t] = 0.0f;
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

// Where the epilogues write in packed mode: row `slot` at rows + slot * variant and its exist value
// into the id record at ids + slot (ids may be nullptr).  The plan left slot -1 past the capacity.
struct C3sOut {
  float* rows;
  C3sPackedRow* ids;
};

// kPacked: a chunk without a slot is skipped whole; the epilogue of a group of one chunk writes to
// po, not into the frame's slot
template <bool kPacked>
__global__ __launch_bounds__(kC3sBlock) void c3s_accum_kernel(const VfTable* __restrict__ T,
                                                              const uint32_t* __restrict__ order,
                                                              const C3sChunk* __restrict__ chunks,
                                                              const uint32_t* __restrict__ cnt, int64_t chunk_cap,
                                                              const uint32_t* __restrict__ lut, C3sThr thr, int stride,
                                                              int col0, unsigned long long* __restrict__ acc, C3sOut po) {
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
    if constexpr (kPacked) {
      if (ch.slot < 0) continue;  // (uniform over the workgroup)
    }
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
      const int32_t exv = exist_from((float)s_ex[0], (float)s_ex[1]);
      const bool ex = exv != 0;
      float* out;
      if constexpr (kPacked) {
        if (tid == 0 && po.ids) po.ids[ch.slot].exist = exv;
        out = po.rows + ch.slot * kC3sBins;
      } else {
        if (tid == 0 && fr.exist) fr.exist[ch.row - T->hpre[f]] = exv;
        out = fr.rows + (ch.row - T->hpre[f]) * stride + col0;
      }
#pragma unroll
      for (int i = 0; i < kC3sBinsPerThread; ++i) {
        const int bin = tid + kC3sBlock * i;
        if (bin < kC3sBins) out[bin] = ex ? (float)sum[i] * norm981(bin) : 0.0f;
      }
    }
  }
}

template <int kBins, bool kPacked>
__global__ __launch_bounds__(256) void c3s_final_kernel(const VfTable* __restrict__ T, const uint32_t* __restrict__ cnt,
                                                        int64_t multi_cap, const int64_t* __restrict__ multi_row,
                                                        const unsigned long long* __restrict__ acc, int stride, int col0,
                                                        const int64_t* __restrict__ multi_slot, C3sOut po) {
  const int64_t nm = std::min<int64_t>((int64_t)cnt[1], multi_cap);
  for (int64_t m = blockIdx.x; m < nm; m += gridDim.x) {
    const unsigned long long* hist = acc + m * kBins;
    const int64_t row = multi_row[m];
    const int f = vf_frame_of(T->hpre, T->nf, row);
    const int32_t exv = exist_from((float)hist[0], (float)hist[1]);
    const bool ex = exv != 0;
    float* out;
    if constexpr (kPacked) {
      const int64_t slot = multi_slot[m];
      if (slot < 0) continue;  // (its chunks added nothing)
      if (threadIdx.x == 0 && po.ids) po.ids[slot].exist = exv;
      out = po.rows + slot * kBins;
    } else {
      if (threadIdx.x == 0 && T->fr[f].exist) T->fr[f].exist[row - T->hpre[f]] = exv;
      out = T->fr[f].rows + (row - T->hpre[f]) * stride + col0;
    }
    for (int i = threadIdx.x; i < kBins; i += 256)
      out[i] = ex ? (float)hist[i] * (kBins == kC3sBins ? norm981(i) : norm117(i)) : 0.0f;
  }
}

// ---- the 117 bins: a chunk per wave ----------------------------------------------------------------
// Per slice of kC3s117Slice voxels three wave-local phases.  Stage: lane = (voxel, position), as
// above.  Fold: lane = voxel, its 13 neighbour words summed per field into the voxel's record
// (c3_sparse.h): the factor 13 leaves the accumulate phase.  Accumulate: lane = bins lane and
// lane + 64, each the product of two fields of the record; the lanes walk the records together.
// Nothing is shared between the waves of a workgroup, so no workgroup barrier is met: a wave's
// LDS writes are ordered before its own later reads by wave_lds_fence.  kPacked: as c3s_accum_kernel.
template <bool kPacked>
__global__ __launch_bounds__(kC3sBlock) void c3s117_accum_kernel(const VfTable* __restrict__ T,
                                                                 const uint32_t* __restrict__ order,
                                                                 const C3sChunk* __restrict__ chunks,
                                                                 const uint32_t* __restrict__ cnt, int64_t chunk_cap,
                                                                 const uint32_t* __restrict__ lut, C3sThr thr, int stride,
                                                                 int col0, unsigned long long* __restrict__ acc, C3sOut po) {
  __shared__ uint64_t s_w[kC3s117Waves][kC3s117Slice * kC3sPos];
  __shared__ uint32_t s_r[kC3s117Waves][kC3s117Slice * kC3s117Words];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t* const sw = s_w[wave];
  uint32_t* const sr = s_r[wave];
  int wx[2], sx[2], wy[2], sy[2];
  uint32_t mx[2], my[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint32_t d = kC3s117Tab.v[lane + 64 * i];
    wx[i] = (int)(d & 7u);
    sx[i] = (int)(d >> 3 & 31u);
    mx[i] = (1u << (d >> 8 & 31u)) - 1u;
    wy[i] = (int)(d >> 13 & 7u);
    sy[i] = (int)(d >> 16 & 31u);
    my[i] = (1u << (d >> 21 & 31u)) - 1u;
  }
  const int64_t nchunks = std::min<int64_t>((int64_t)cnt[0], chunk_cap);
  for (int64_t ci = (int64_t)blockIdx.x * kC3s117Waves + wave; ci < nchunks; ci += (int64_t)gridDim.x * kC3s117Waves) {
    const C3sChunk ch = chunks[ci];
    if constexpr (kPacked) {
      if (ch.slot < 0) continue;  // (uniform over the wave; no workgroup barrier is met)
    }
    const int f = vf_frame_of(T->hpre, T->nf, ch.row);
    const VfFrame& fr = T->fr[f];
    const GrsdArgs& ga = fr.ga;
    const int32_t* __restrict__ vk = fr.vkeys;
    const int64_t nc = ga.nc, v0 = T->vpre[f];
    uint32_t sum[2] = {0u, 0u};
    for (uint32_t s0 = 0; s0 < ch.count; s0 += kC3s117Slice) {
      const int m = (int)std::min<uint32_t>(kC3s117Slice, ch.count - s0);
      wave_lds_fence();  // the phases of the slice before have read sw and sr
      __builtin_amdgcn_wave_barrier();
      for (int e = lane; e < m * kC3sPos; e += 64) {
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
              const int64_t own = vk[v], off = lin - own;  // (the bounds of c3s_accum_kernel's search)
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
        sw[e] = w;
      }
      wave_lds_fence();
      __builtin_amdgcn_wave_barrier();
      if (lane < m) {
        const uint64_t* w = sw + lane * kC3sPos;
        // the centre's staged word is words 0 and 1 of the record as it stands
        uint32_t n[6] = {0u, 0u, 0u, 0u, 0u, 0u}, b = 0u;
#pragma unroll
        for (int p = 1; p < kC3sPos; ++p) {
          const uint64_t x = w[p];
#pragma unroll
          for (int c = 0; c < 6; ++c) n[c] += (uint32_t)(x >> (8 * c)) & 0xffu;
          // beta bits 48 .. 53 spread to 4-bit fields: 13 ones at most per field
          const uint32_t be = (uint32_t)(x >> 48) & 0x3fu;
#pragma unroll
          for (int c = 0; c < 6; ++c) b += (be >> c & 1u) << (4 * c);
        }
        uint32_t* r = sr + lane * kC3s117Words;
        r[0] = (uint32_t)w[0];
        r[1] = (uint32_t)(w[0] >> 32);
        r[2] = n[0] | n[1] << 16;
        r[3] = n[2] | n[3] << 16;
        r[4] = n[4] | n[5] << 16;
        r[5] = b;
      }
      wave_lds_fence();
      __builtin_amdgcn_wave_barrier();
      for (int j = 0; j < m; ++j) {
        const uint32_t* r = sr + j * kC3s117Words;
#pragma unroll
        for (int i = 0; i < 2; ++i) sum[i] += ((r[wx[i]] >> sx[i]) & mx[i]) * ((r[wy[i]] >> sy[i]) & my[i]);
      }
    }
    if (ch.multi >= 0) {
      unsigned long long* slot = acc + (int64_t)ch.multi * kC3s117Bins;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int bin = lane + 64 * i;
        if (bin < kC3s117Bins && sum[i]) atomicAdd(&slot[bin], (unsigned long long)sum[i]);
      }
    } else {
      const int32_t exv = exist_from((float)__shfl(sum[0], 0, 64), (float)__shfl(sum[0], 1, 64));
      const bool ex = exv != 0;
      float* out;
      if constexpr (kPacked) {
        if (lane == 0 && po.ids) po.ids[ch.slot].exist = exv;
        out = po.rows + ch.slot * kC3s117Bins;
      } else {
        if (lane == 0 && fr.exist) fr.exist[ch.row - T->hpre[f]] = exv;
        out = fr.rows + (ch.row - T->hpre[f]) * stride + col0;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int bin = lane + 64 * i;
        if (bin < kC3s117Bins) out[bin] = ex ? (float)sum[i] * norm117(bin) : 0.0f;
      }
    }
  }
}

// The packed pass (C3sPack, c3h_internal.h).  kC3sPackPlan: keys, sort, the heads of the tiles, their
// scan, the frames' first positions, the plan with slots.  kC3sPackAccum: the accumulate launches
// with packed epilogues.  c3s_fill_kernel is not launched: no row it would zero is written.
hipError_t launch_c3_packed(const VfTable* d_tab, int64_t vtot, int64_t htot, const C3sBufs& b, const uint32_t* lut,
                            const int32_t thr[3], int variant, hipStream_t s, const C3sPack& pk) {
  if (vtot <= 0) return hipErrorInvalidValue;  // (a batch with a row has a voxel)
  const int64_t chunk_cap = c3s_chunk_cap(vtot, htot), multi_cap = c3s_multi_cap(vtot), ntiles = c3s_plan_tiles(vtot);
  const int tblocks = (int)std::min<int64_t>(ntiles, 8192);
  hipError_t e = hipSuccess;
  if (pk.phases & kC3sPackPlan) {
    e = hipMemsetAsync(b.cnt, 0, 2 * sizeof(uint32_t), s);
    if (e == hipSuccess && multi_cap > 0) e = hipMemsetAsync(b.acc, 0, (size_t)multi_cap * variant * 8, s);
    if (e != hipSuccess) return e;
    c3s_keys_kernel<<<c3s_blocks(vtot), 256, 0, s>>>(d_tab, vtot, htot, b.keys, b.idx);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = *b.tmp_bytes;
    e = rocprim::radix_sort_pairs(b.tmp, bytes, b.keys, b.keys2, b.idx, b.idx2, (size_t)vtot, 0, c3s_key_bits(htot), s);
    if (e != hipSuccess) return e;
    c3s_pack_count_kernel<<<tblocks, 256, 0, s>>>(b.keys2, vtot, htot, pk.tile_heads);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    c3s_pack_scan_kernel<<<1, 256, 0, s>>>(pk.tile_heads, ntiles, pk.tile_base);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    c3s_pack_frames_kernel<<<pk.nf + 1, 256, 0, s>>>(d_tab, b.keys2, vtot, pk.tile_base, pk.frame_first);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    c3s_plan_kernel<true><<<tblocks, 256, 0, s>>>(b.keys2, vtot, htot, chunk_cap, multi_cap, b.cnt, b.chunks, b.multi_row,
                                                   pk.tile_base, pk.base, pk.multi_slot, d_tab, pk.ids, pk.cap, pk.frame0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (!(pk.phases & kC3sPackAccum)) return e;
  const C3sOut po{pk.rows, pk.ids};
  C3sThr t;
  for (int a = 0; a < 3; ++a) t.v[a] = thr[a];
  if (variant == kC3s117Bins) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((chunk_cap + kC3s117Waves - 1) / kC3s117Waves, 4096));
    c3s117_accum_kernel<true><<<blocks, kC3sBlock, 0, s>>>(d_tab, b.idx2, b.chunks, b.cnt, chunk_cap, lut, t, 0, 0, b.acc, po);
  } else {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(chunk_cap, 4096));
    c3s_accum_kernel<true><<<blocks, kC3sBlock, 0, s>>>(d_tab, b.idx2, b.chunks, b.cnt, chunk_cap, lut, t, 0, 0, b.acc, po);
  }
  e = hipGetLastError();
  if (e != hipSuccess || multi_cap == 0) return e;
  const int fblocks = (int)std::min<int64_t>(multi_cap, 4096);
  if (variant == kC3s117Bins)
    c3s_final_kernel<kC3s117Bins, true><<<fblocks, 256, 0, s>>>(d_tab, b.cnt, multi_cap, b.multi_row, b.acc, 0, 0, pk.multi_slot, po);
  else
    c3s_final_kernel<kC3sBins, true><<<fblocks, 256, 0, s>>>(d_tab, b.cnt, multi_cap, b.multi_row, b.acc, 0, 0, pk.multi_slot, po);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_c3_sparse(const VfTable* d_tab, int64_t vtot, int64_t htot, const C3sBufs& b, const uint32_t* lut,
                            const int32_t thr[3], int variant, int stride, int col0, hipStream_t s, const C3sPack* pk) {
  const size_t n = (size_t)std::max<int64_t>(vtot, 1);
  const int bits = c3s_key_bits(htot);
  if (!b.tmp) {  // size query
    size_t bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, b.keys, b.keys2, b.idx, b.idx2, n, 0, bits, s);
    *b.tmp_bytes = bytes;
    return e;
  }
  if (variant != kC3sBins && variant != kC3s117Bins) return hipErrorInvalidValue;
  if (htot <= 0) return hipSuccess;
  if (pk) return launch_c3_packed(d_tab, vtot, htot, b, lut, thr, variant, s, *pk);
  if (variant == kC3s117Bins)  // (4,096 workgroups: 16,384 rows a sweep, as at 981)
    c3s_fill_kernel<4><<<(int)std::min<int64_t>((htot + 3) / 4, 4096), 256, 0, s>>>(d_tab, htot, variant, stride, col0);
  else
    c3s_fill_kernel<1><<<(int)std::min<int64_t>(htot, 16384), 256, 0, s>>>(d_tab, htot, variant, stride, col0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || vtot <= 0) return e;
  const int64_t chunk_cap = c3s_chunk_cap(vtot, htot), multi_cap = c3s_multi_cap(vtot);
  e = hipMemsetAsync(b.cnt, 0, 2 * sizeof(uint32_t), s);
  if (e == hipSuccess && multi_cap > 0) e = hipMemsetAsync(b.acc, 0, (size_t)multi_cap * variant * 8, s);
  if (e != hipSuccess) return e;
  c3s_keys_kernel<<<c3s_blocks(vtot), 256, 0, s>>>(d_tab, vtot, htot, b.keys, b.idx);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  size_t bytes = *b.tmp_bytes;
  e = rocprim::radix_sort_pairs(b.tmp, bytes, b.keys, b.keys2, b.idx, b.idx2, (size_t)vtot, 0, bits, s);
  if (e != hipSuccess) return e;
  c3s_plan_kernel<false><<<(int)std::min<int64_t>((vtot + kC3sPlanTile - 1) / kC3sPlanTile, 8192), 256, 0, s>>>(b.keys2, vtot, htot, chunk_cap, multi_cap, b.cnt, b.chunks, b.multi_row, nullptr, 0, nullptr, nullptr, nullptr, 0, 0);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const C3sOut none{nullptr, nullptr};
  C3sThr t;
  for (int a = 0; a < 3; ++a) t.v[a] = thr[a];
  if (variant == kC3s117Bins) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((chunk_cap + kC3s117Waves - 1) / kC3s117Waves, 4096));
    c3s117_accum_kernel<false><<<blocks, kC3sBlock, 0, s>>>(d_tab, b.idx2, b.chunks, b.cnt, chunk_cap, lut, t, stride, col0, b.acc, none);
  } else {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(chunk_cap, 4096));
    c3s_accum_kernel<false><<<blocks, kC3sBlock, 0, s>>>(d_tab, b.idx2, b.chunks, b.cnt, chunk_cap, lut, t, stride, col0, b.acc, none);
  }
  e = hipGetLastError();
  if (e != hipSuccess || multi_cap == 0) return e;
  const int fblocks = (int)std::min<int64_t>(multi_cap, 4096);
  if (variant == kC3s117Bins)
    c3s_final_kernel<kC3s117Bins, false><<<fblocks, 256, 0, s>>>(d_tab, b.cnt, multi_cap, b.multi_row, b.acc, stride, col0, nullptr, none);
  else
    c3s_final_kernel<kC3sBins, false><<<fblocks, 256, 0, s>>>(d_tab, b.cnt, multi_cap, b.multi_row, b.acc, stride, col0, nullptr, none);
  return hipGetLastError();
}

}  // namespace c3h
