// c3_sparse.h -- host arithmetic of the sparse batched C3-HLAC-981 / 117 (c3_sparse.hip): the sort
// key that groups a batch's voxels by output row, the chunk plan of a group, the packed position of a
// group (the packed output), the subdivision of an acting cell, and the inverses of the 981-bin and
// 117-bin layouts as the tables the accumulate phases read.  Plain C++: the kernels (c3_sparse.hip),
// the launch code (capi_vosch.hip) and the host checks (tests/c3_sparse_check.cpp,
// tests/c3_rows_check.cpp, tests/packed_rows_check.cpp) include it.
#pragma once
#include <cmath>
#include <cstdint>

#include "vosch_frames.h"

namespace c3h {

constexpr int kC3sBlock = 256;          // threads of the accumulate workgroup
constexpr int kC3sSlice = 128;          // voxels staged in LDS at a time
constexpr int kC3sChunk = 1024;         // voxels of one workgroup's chunk: its sums stay in u32 registers
constexpr int kC3sBins = 981;
constexpr int kC3sBinsPerThread = (kC3sBins + kC3sBlock - 1) / kC3sBlock;
constexpr int kC3sPos = 14;             // staged words per voxel: the centre and its 13 neighbours
static_assert((uint64_t)kC3sChunk * 65025 < ((uint64_t)1 << 32), "a chunk's largest sum (255 * 255 per voxel) fits u32");
static_assert(kC3sChunk % kC3sSlice == 0, "a chunk is whole slices");

// ---- the sort key ------------------------------------------------------------------------------
// key = hpre[frame] + subdivision: the row's ordinal in the batch, so keys order by (frame,
// subdivision).  The value htot (one past the last row) marks a voxel that feeds no row; it sorts
// last.  Sorted on c3s_key_bits(htot) bits of a 64-bit word.
C3H_VF_HD inline uint64_t c3s_none(int64_t htot) { return (uint64_t)htot; }
C3H_VF_HD inline uint64_t c3s_key(const int64_t* hpre, int frame, int64_t sub) { return (uint64_t)(hpre[frame] + sub); }
inline int c3s_key_bits(int64_t htot) { return vf_bits((uint64_t)htot); }

// ---- the chunk plan ----------------------------------------------------------------------------
// A group (the voxels of one row, consecutive after the sort) of L voxels is cut into
// c3s_chunks(L) chunks of at most kC3sChunk; chunk i holds c3s_chunk_len(L, i) voxels from
// i * kC3sChunk.  A group of several chunks adds 64-bit partial sums.
C3H_VF_HD inline int64_t c3s_chunks(int64_t L) { return (L + kC3sChunk - 1) / kC3sChunk; }
C3H_VF_HD inline int64_t c3s_chunk_len(int64_t L, int64_t i) {
  const int64_t r = L - i * kC3sChunk;
  return r < 0 ? 0 : (r > kC3sChunk ? kC3sChunk : r);
}
// upper bounds known without reading the device: chunks (every group adds floor(L / chunk) full
// ones and at most one more) and groups of several chunks (each holds more than a chunk)
inline int64_t c3s_chunk_cap(int64_t vtot, int64_t htot) { return vtot / kC3sChunk + (vtot < htot ? vtot : htot); }
inline int64_t c3s_multi_cap(int64_t vtot) { return vtot / (kC3sChunk + 1); }

struct C3sChunk {
  int64_t row;      // the batch ordinal of the output row
  uint32_t start;   // first sorted position
  uint32_t count;   // voxels, 1 .. kC3sChunk
  int32_t multi;    // the ordinal of its group among those of several chunks, or -1
  int32_t pad;
  int64_t slot;     // packed mode: the packed position of its group's row in the call; else -1
};

// ---- the packed output ---------------------------------------------------------------------------
// c3h_extract_c3_frames_packed writes only the rows that hold a voxel, in the order of the sorted
// keys (frame, then row ordinal): the packed position of a group is the number of group heads in
// front of it.  A head is a sorted position whose key is a row's and differs from the key before.
// The plan works on tiles of kC3sPlanTile sorted positions, a workgroup of 256 threads a tile,
// thread tid at the positions t * tile + it * 256 + tid (it = 0 .. kC3sPlanItems - 1).  Three
// launches give every head its ordinal without a workgroup waiting on another: the heads of every
// tile (c3s_pack_count), an exclusive scan of those totals by one workgroup (c3s_pack_scan), and in
// the plan the heads in front within the tile: the whole rounds before `it` and, of round `it`,
// the waves before this one and the lanes of this wave's ballot below this lane.
constexpr int kC3sPlanItems = 8;
constexpr int kC3sPlanTile = 256 * kC3sPlanItems;
constexpr int kC3sPlanWaves = 4;

struct C3sPackedRow {  // c3h_packed_row (c3hlac_mi355x.h)
  int32_t frame;       // the frame's index in the call
  int32_t exist;       // exist_voxel_num of the row
  int64_t row;         // the row's ordinal in its frame
};
static_assert(sizeof(C3sPackedRow) == 16, "the id record is 16 bytes");

C3H_VF_HD inline bool c3s_head(const uint64_t* keys, int64_t i, uint64_t none) {
  const uint64_t k = keys[i];
  return k < none && (i == 0 || keys[i - 1] != k);
}
C3H_VF_HD inline int64_t c3s_plan_tiles(int64_t vtot) { return (vtot + kC3sPlanTile - 1) / kC3sPlanTile; }
C3H_VF_HD inline int64_t c3s_plan_pos(int64_t t, int it, int tid) { return t * kC3sPlanTile + it * 256 + tid; }
// heads of the tile in front of (round it, wave, lane): wave_heads[it' * kC3sPlanWaves + w] = the
// heads of wave w in round it', ballot = the head lanes of this wave in round it
C3H_VF_HD inline uint32_t c3s_pack_local(const uint32_t* wave_heads, int it, int wave, uint64_t ballot, int lane) {
  uint32_t n = 0;
  for (int j = 0; j < it * kC3sPlanWaves + wave; ++j) n += wave_heads[j];
  const uint64_t below = ballot & (((uint64_t)1 << lane) - 1);
  for (uint64_t b = below; b; b &= b - 1) ++n;
  return n;
}
// the packed position in the call: the rows of the batches before, the tiles before, the heads before
C3H_VF_HD inline int64_t c3s_pack_slot(int64_t base, int64_t tile_base, uint32_t local) { return base + tile_base + local; }
// a row at `slot` is written (and its chunks are computed) only inside the caller's capacity
C3H_VF_HD inline bool c3s_slot_written(int64_t slot, int64_t cap) { return slot < cap; }

// exist_from (c3hlac_dev.h) on the host: exist_voxel_num from the sums of bins 0 and 1
inline int32_t c3s_exist_of(float s0, float s1) {
  const float n0 = (float)(1 / 255.0);
  const float f0 = s0 * n0;
  const float f1 = s1 * n0;
  const float t = (f0 + f1) * 2.0f;
  return (int32_t)((double)t + 0.001);
}

// ---- the subdivision of an acting cell ---------------------------------------------------------
// c3_hlac.cpp:349-356 as offcell_contrib (c3hlac.hip) has it: a = floor(c / leaf) - min_b.  One
// row: histogram 0 whatever the cell.  Else t = a - offset, skipped below 0; floorf((float)t *
// inv_s) per axis, dropped from sb on.  Returns the subdivision or -1.
C3H_VF_HD inline int64_t c3s_subdivision(const int a[3], const int off[3], const int sb[3], float inv_s, int hist1) {
  if (hist1) return 0;
  int ijk[3];
  for (int ax = 0; ax < 3; ++ax) {
    const int t = a[ax] - off[ax];
    if (t < 0) return -1;
    ijk[ax] = (int)floorf((float)t * inv_s);
    if (ijk[ax] >= sb[ax]) return -1;
  }
  return ijk[0] + (int64_t)sb[0] * (ijk[1] + (int64_t)sb[1] * ijk[2]);
}

// relative coordinates of neighbour k (c3_hlac.cpp:177-202)
C3H_VF_HD inline void c3s_rel(int k, int rel[3]) {
  rel[0] = k < 9 ? k / 3 - 1 : (k < 12 ? k - 10 : -1);
  rel[1] = k < 9 ? k % 3 - 1 : (k < 12 ? -1 : 0);
  rel[2] = k < 9 ? -1 : 0;
}

// ---- the bins ------------------------------------------------------------------------------------
// The closed form of the layout (bin981 / tri6 of c3hlac_dev.h)
C3H_VF_HD constexpr int c3s_bin981(int k, int c, int n) {
  return k <= 8 ? 6 + 78 * c + 9 * n + k : 60 + 78 * c + 4 * n + (k - 9);
}
C3H_VF_HD constexpr int c3s_tri6(int c, int n) { return 6 * c - c * (c - 1) / 2 + (n - c); }

// A staged voxel word (centre or neighbour; 0 = absent): bytes 0 .. 5 the channel values a[0 .. 5],
// bits 48 .. 53 the binarised beta[0 .. 5], bit 63 set.  A field of it is (word >> shift) & mask.
// Every bin is the sum over the group's voxels of field A of the centre times field B of one
// position (the centre again for the zero-order and auto-product bins).
enum { kC3sFieldBeta = 6, kC3sFieldOne = 12 };  // fields 0 .. 5: a[c]; 6 .. 11: beta[c]; 12: the constant 1
C3H_VF_HD constexpr int c3s_field_shift(int f) { return f < 6 ? 8 * f : (f < 12 ? 48 + (f - 6) : 63); }
C3H_VF_HD constexpr uint32_t c3s_field_mask(int f) { return f < 6 ? 0xffu : 1u; }

struct C3sBin {
  int pos;     // 0: the centre; 1 + k: neighbour k
  int fa, fb;  // the centre's field, the position's field
};
// the inverse of the layout: what bin i sums
C3H_VF_HD constexpr C3sBin c3s_bin_desc(int i) {
  const int type = i >= 495 ? 1 : 0;  // 1: the binarised half
  const int j = type ? i - 495 : i;
  const int fo = type ? kC3sFieldBeta : 0;
  if (j < 6) return C3sBin{0, fo + j, kC3sFieldOne};
  if (j < 474) {
    const int c = (j - 6) / 78, r = (j - 6) % 78;
    const int n = r < 54 ? r / 9 : (r - 54) / 4;
    const int k = r < 54 ? r % 9 : 9 + (r - 54) % 4;
    return C3sBin{1 + k, fo + c, fo + n};
  }
  if (!type) {  // 474 .. 494: the auto-product triangle a[c] * a[n], c <= n
    int t = j - 474, c = 0;
    while (t >= 6 - c) {
      t -= 6 - c;
      ++c;
    }
    return C3sBin{0, c, c + t};
  }
  const int t = j - 474;  // 969 .. 980: the twelve binarised channel pairs
  if (t < 8) return C3sBin{0, kC3sFieldBeta + t / 4, kC3sFieldBeta + 2 + t % 4};
  return C3sBin{0, kC3sFieldBeta + 2 + (t - 8) / 2, kC3sFieldBeta + 4 + (t - 8) % 2};
}

// The table of the accumulate phase, a word per bin:
// pos | shift A << 4 | shift B << 10 | (mask A is 0xff) << 16 | (mask B is 0xff) << 17 | 1 << 18
C3H_VF_HD constexpr uint32_t c3s_pack_bin(const C3sBin& b) {
  return (uint32_t)b.pos | (uint32_t)c3s_field_shift(b.fa) << 4 | (uint32_t)c3s_field_shift(b.fb) << 10 |
         (c3s_field_mask(b.fa) == 0xffu ? 1u << 16 : 0u) | (c3s_field_mask(b.fb) == 0xffu ? 1u << 17 : 0u) | 1u << 18;
}
struct C3sTable {
  uint32_t v[kC3sBlock * kC3sBinsPerThread];  // 0 past bin 980: both masks 0
};
constexpr C3sTable c3s_make_table() {
  C3sTable t{};
  for (int i = 0; i < kC3sBins; ++i) t.v[i] = c3s_pack_bin(c3s_bin_desc(i));
  return t;
}

// ---- the 117 bins (the rotation-invariant variant) -------------------------------------------------
// fold117's layout (c3hlac_dev.h): every first-order bin sums its 13 neighbour positions, so with
// N[n] = sum over the 13 neighbours of a[n] and B[n] = the same of beta[n], every one of the 117 bins
// is the sum over the group's voxels of field X times field Y of one record per voxel:
//   field 0: the constant 1;  1 .. 6: a[c];  7 .. 12: beta[c];  13 .. 18: N[n];  19 .. 24: B[n]
// (w117_bin_channels' numbering).  a <= 255, N <= 13 * 255 = 3,315, beta <= 1, B <= 13.
constexpr int kC3s117Bins = 117;
constexpr int kC3s117Fields = 25;
constexpr int kC3s117Words = 6;   // 32-bit words of a voxel's record
constexpr int kC3s117Slice = 64;  // voxels a wave stages at a time: a lane per voxel in the fold
constexpr int kC3s117Waves = kC3sBlock / 64;  // a chunk per wave
static_assert(kC3s117Bins <= 128, "two bins per lane of one wave");
static_assert((uint64_t)13 * kC3sChunk * 65025 < ((uint64_t)1 << 32),
              "a chunk's largest 117 sum (13 neighbours x 255 x 255 per voxel) fits u32");
static_assert(kC3sChunk % kC3s117Slice == 0, "a chunk is whole slices");

// The record: word 0: a[0 .. 3] as bytes; word 1: a[4], a[5] as bytes, beta[0 .. 5] in bits 16 .. 21,
// bit 31 set (the constant 1); words 2 .. 4: N[0 .. 5], 16 bits each; word 5: B[0 .. 5], 4 bits each
C3H_VF_HD constexpr int c3s117_field_word(int f) {
  return f == 0 ? 1 : f < 7 ? (f - 1) / 4 : f < 13 ? 1 : f < 19 ? 2 + (f - 13) / 2 : 5;
}
C3H_VF_HD constexpr int c3s117_field_shift(int f) {
  return f == 0 ? 31 : f < 7 ? 8 * ((f - 1) % 4) : f < 13 ? 16 + (f - 7) : f < 19 ? 16 * ((f - 13) % 2) : 4 * (f - 19);
}
C3H_VF_HD constexpr int c3s117_field_bits(int f) { return f == 0 ? 1 : f < 7 ? 8 : f < 13 ? 1 : f < 19 ? 16 : 4; }

struct C3s117Bin {
  int fx, fy;  // the two fields whose product the bin sums
};
// the inverse of fold117's layout: what bin i sums
C3H_VF_HD constexpr C3s117Bin c3s117_bin_desc(int i) {
  if (i < 6) return C3s117Bin{0, 1 + i};                            // zero order
  if (i < 42) return C3s117Bin{1 + (i - 6) / 6, 13 + (i - 6) % 6};  // a[c] * N[n]
  if (i < 63) {                                                     // the auto-product triangle a[c] * a[n], c <= n
    int t = i - 42, c = 0;
    while (t >= 6 - c) {
      t -= 6 - c;
      ++c;
    }
    return C3s117Bin{1 + c, 1 + c + t};
  }
  if (i < 69) return C3s117Bin{0, 7 + (i - 63)};                      // binarised zero order
  if (i < 105) return C3s117Bin{7 + (i - 69) / 6, 19 + (i - 69) % 6};  // beta[c] * B[n]
  const int t = i - 105;                                              // the twelve binarised channel pairs
  if (t < 8) return C3s117Bin{7 + t / 4, 7 + 2 + t % 4};
  return C3s117Bin{7 + 2 + (t - 8) / 2, 7 + 4 + (t - 8) % 2};
}
// the 117 bin that fold117 adds 981-bin j into
C3H_VF_HD constexpr int c3s117_of_981(int j) {
  const int type = j >= 495 ? 1 : 0, r = type ? j - 495 : j;
  if (r < 6) return (type ? 63 : 0) + r;
  if (r < 474) return (type ? 69 : 6) + 6 * ((r - 6) / 78) + ((r - 6) % 78 < 54 ? (r - 6) % 78 / 9 : ((r - 6) % 78 - 54) / 4);
  return (type ? 105 : 42) + (r - 474);
}

// The table of the 117 accumulate phase, a word per bin:
// word X | shift X << 3 | bits X << 8 | word Y << 13 | shift Y << 16 | bits Y << 21 | 1 << 26
C3H_VF_HD constexpr uint32_t c3s117_pack_bin(const C3s117Bin& b) {
  return (uint32_t)c3s117_field_word(b.fx) | (uint32_t)c3s117_field_shift(b.fx) << 3 | (uint32_t)c3s117_field_bits(b.fx) << 8 |
         (uint32_t)c3s117_field_word(b.fy) << 13 | (uint32_t)c3s117_field_shift(b.fy) << 16 |
         (uint32_t)c3s117_field_bits(b.fy) << 21 | 1u << 26;
}
struct C3s117Table {
  uint32_t v[128];  // 0 past bin 116: both fields of 0 bits
};
constexpr C3s117Table c3s117_make_table() {
  C3s117Table t{};
  for (int i = 0; i < kC3s117Bins; ++i) t.v[i] = c3s117_pack_bin(c3s117_bin_desc(i));
  return t;
}

}  // namespace c3h
