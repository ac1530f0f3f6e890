// packed_rows_check.cpp -- the pack arithmetic of the sparse C3-HLAC pass (csrc/c3_sparse.h) on the
// host (its own main; built with -fsanitize=address,undefined by test_packed_rows_cpu.py).
//
// The packed position of a row is the number of group heads in front of it in the sorted keys.  The
// kernels get it in three steps (c3s_pack_count, c3s_pack_scan, c3s_plan_kernel<true>): the heads
// of every plan tile, an exclusive scan of the tiles, and inside a tile the heads of the rounds and
// waves in front and of the lanes below in the wave's ballot.  Here the same steps run on the key
// sequences of the ladders (c3_sparse_data.py: LADDER_A, LADDER_B, both arrangements, with and
// without "none" keys and an empty row) and of a tile-crossing run of one-voxel groups, through
// c3_sparse.h's own functions, and are compared with the plain count; the frames' first positions
// likewise.  Then slot against capacity, and that a group that holds a voxel has exist >= 1 for all
// 256 channel values x 3 colour modes -- why packing by group is packing by exist > 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "c3_sparse.h"
#include "colour_lut.h"

static long n_head = 0, n_seq = 0, n_value = 0;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

// the sorted keys of a batch: per frame its rows' lengths (0: an empty row), `none` voxels that feed
// no row behind all groups
static std::vector<uint64_t> keys_of(const std::vector<std::vector<int>>& frames, int none, std::vector<int64_t>* hpre) {
  std::vector<uint64_t> keys;
  hpre->assign(1, 0);
  for (const auto& lens : frames) {
    for (size_t h = 0; h < lens.size(); ++h)
      for (int v = 0; v < lens[h]; ++v) keys.push_back(c3h::c3s_key(hpre->data(), (int)hpre->size() - 1, (int64_t)h));
    hpre->push_back(hpre->back() + (int64_t)lens.size());
  }
  for (int v = 0; v < none; ++v) keys.push_back(c3h::c3s_none(hpre->back()));
  return keys;
}

static void check_sequence(const std::vector<std::vector<int>>& frames, int none, int64_t base, int64_t cap) {
  std::vector<int64_t> hpre;
  const std::vector<uint64_t> keys = keys_of(frames, none, &hpre);
  const int64_t vtot = (int64_t)keys.size(), htot = hpre.back(), ntiles = c3h::c3s_plan_tiles(vtot);
  const uint64_t no = c3h::c3s_none(htot);
  CHECK(vtot > 0);
  // the plain count: ordinal[i] for every head i
  std::vector<int64_t> ordinal((size_t)vtot, -1);
  int64_t heads = 0, rows_with_voxel = 0;
  for (int64_t i = 0; i < vtot; ++i)
    if (c3h::c3s_head(keys.data(), i, no)) ordinal[(size_t)i] = heads++;
  for (const auto& lens : frames)
    for (int L : lens) rows_with_voxel += L > 0;
  CHECK(heads == rows_with_voxel);  // a head per row that holds a voxel, none for the "none" keys
  // 1. the heads of every tile (c3s_pack_count_kernel: a ballot per round and wave)
  std::vector<uint32_t> tile_heads((size_t)ntiles, 0);
  std::vector<std::vector<uint32_t>> wave_heads((size_t)ntiles, std::vector<uint32_t>(c3h::kC3sPlanItems * c3h::kC3sPlanWaves, 0));
  std::vector<std::vector<uint64_t>> ballots((size_t)ntiles, std::vector<uint64_t>(c3h::kC3sPlanItems * c3h::kC3sPlanWaves, 0));
  for (int64_t t = 0; t < ntiles; ++t)
    for (int it = 0; it < c3h::kC3sPlanItems; ++it)
      for (int tid = 0; tid < 256; ++tid) {
        const int64_t i = c3h::c3s_plan_pos(t, it, tid);
        if (i < vtot && c3h::c3s_head(keys.data(), i, no)) {
          ++tile_heads[(size_t)t];
          ++wave_heads[(size_t)t][it * c3h::kC3sPlanWaves + tid / 64];
          ballots[(size_t)t][it * c3h::kC3sPlanWaves + tid / 64] |= (uint64_t)1 << (tid % 64);
        }
      }
  // every position of a tile is visited once, in ascending order of (it, tid)
  CHECK(c3h::c3s_plan_pos(1, 0, 0) == c3h::kC3sPlanTile && c3h::c3s_plan_pos(0, c3h::kC3sPlanItems - 1, 255) == c3h::kC3sPlanTile - 1);
  CHECK(c3h::c3s_plan_pos(0, 1, 0) == c3h::c3s_plan_pos(0, 0, 255) + 1);
  // 2. the exclusive scan (c3s_pack_scan_kernel)
  std::vector<int64_t> tile_base((size_t)ntiles + 1, 0);
  for (int64_t t = 0; t < ntiles; ++t) tile_base[(size_t)t + 1] = tile_base[(size_t)t] + tile_heads[(size_t)t];
  CHECK(tile_base[(size_t)ntiles] == heads);
  // 3. the slot of every head (c3s_plan_kernel<true>), against the plain count; slot against capacity
  int64_t written = 0;
  for (int64_t t = 0; t < ntiles; ++t)
    for (int it = 0; it < c3h::kC3sPlanItems; ++it)
      for (int tid = 0; tid < 256; ++tid) {
        const int64_t i = c3h::c3s_plan_pos(t, it, tid);
        if (i >= vtot || !c3h::c3s_head(keys.data(), i, no)) continue;
        const int wave = tid / 64, lane = tid % 64;
        const uint32_t local = c3h::c3s_pack_local(wave_heads[(size_t)t].data(), it, wave, ballots[(size_t)t][it * c3h::kC3sPlanWaves + wave], lane);
        const int64_t slot = c3h::c3s_pack_slot(base, tile_base[(size_t)t], local);
        CHECK(slot == base + ordinal[(size_t)i]);
        CHECK(c3h::c3s_slot_written(slot, cap) == (slot < cap));
        written += c3h::c3s_slot_written(slot, cap);
        ++n_head;
      }
  CHECK(written == std::max<int64_t>(0, std::min(heads, cap - base)));  // the rows below the capacity, no other
  // the frames' first positions (c3s_pack_frames_kernel): the heads in front of the first key >= hpre[f]
  int64_t before = 0;
  for (size_t f = 0; f < hpre.size(); ++f) {
    const int64_t lo = std::lower_bound(keys.begin(), keys.end(), (uint64_t)hpre[f]) - keys.begin();
    const int64_t t = lo / c3h::kC3sPlanTile;
    int64_t n = 0;
    for (int it = 0; it < c3h::kC3sPlanItems; ++it)
      for (int tid = 0; tid < 256; ++tid) {
        const int64_t i = c3h::c3s_plan_pos(t, it, tid);
        n += i < lo && c3h::c3s_head(keys.data(), i, no);
      }
    CHECK(t <= ntiles && tile_base[(size_t)t] + n == before);
    if (f + 1 < hpre.size())
      for (int L : frames[f]) before += L > 0;
  }
  CHECK(before == heads);
  ++n_seq;
}

static void check_ladders() {
  const std::vector<int> A = {2047, 2, 2047, 1024, 1025, 2048, 0, 1023, 128, 129, 127, 1, 2049, 5};  // LADDER_A
  const std::vector<int> B = {129, 1024, 0, 767, 127, 1};                                             // LADDER_B
  // at offset (0, 1, 0) the cells of y = 0 feed no row: a row of at most 13 voxels loses them all
  auto off = [](std::vector<int> lens, int* none) {
    *none = 0;
    for (int& L : lens) {
      int lost = 0;
      for (int i = 0; i < L; ++i) lost += (i / 13) % 13 == 0;
      *none += lost;
      L -= lost;
    }
    return lens;
  };
  int na = 0, nb = 0;
  const std::vector<int> A1 = off(A, &na), B1 = off(B, &nb);
  CHECK(std::count_if(A.begin(), A.end(), [](int L) { return L > 0; }) == 13);
  CHECK(std::count_if(A1.begin(), A1.end(), [](int L) { return L > 0; }) == 10);
  CHECK(std::count_if(B.begin(), B.end(), [](int L) { return L > 0; }) == 5);
  CHECK(std::count_if(B1.begin(), B1.end(), [](int L) { return L > 0; }) == 4);
  for (int64_t cap : {(int64_t)1 << 40, (int64_t)17, (int64_t)1, (int64_t)0})
    for (int64_t base : {(int64_t)0, (int64_t)7, ((int64_t)1 << 33) + 5}) {
      const int64_t c = cap == ((int64_t)1 << 40) ? cap : base + cap;
      check_sequence({A}, 0, base, c);
      check_sequence({A, B}, 0, base, c);
      check_sequence({B, A}, 0, base, c);
      check_sequence({A1}, na, base, c);
      check_sequence({B1, A1}, na + nb, base, c);
      check_sequence({A1, B1}, na + nb, base, c);
      check_sequence({B, {}, A, {0, 0}}, 3, base, c);  // a frame without a row, a frame of empty rows
    }
  // one-voxel groups over several tiles (many_rows' shape): every position a head
  std::vector<int> ones(3 * c3h::kC3sPlanTile + 251, 1);
  ones[100] = 0;
  ones[c3h::kC3sPlanTile] = 0;
  check_sequence({ones}, 0, 0, (int64_t)1 << 40);
  check_sequence({ones, B}, 40, 11, 5000);
}

// a group that holds a voxel has exist >= 1: bins 0 and 1 sum a[0] and a[1] of its voxels (the LUT's
// pair of the red byte), and one voxel alone already gives (int)((a0 + a1) / 255 * 2 + 0.001) >= 1
static void check_exist() {
  for (int mode : {C3H_COLOR_C3_FLOAT, C3H_COLOR_C3_DOUBLE, C3H_COLOR_CHLAC}) {
    uint32_t lut[256];
    c3h::host_lut(mode, lut);
    for (int v = 0; v < 256; ++v) {
      const uint32_t a0 = lut[v] & 0xffu, a1 = lut[v] >> 8 & 0xffu;
      CHECK(c3h::c3s_exist_of((float)a0, (float)a1) >= 1);
      // sums only grow with more voxels: the smallest pair 1,024 times, and with the 64-bit sums' floats
      CHECK(c3h::c3s_exist_of((float)(1024u * a0), (float)(1024u * a1)) >= 1);
      ++n_value;
    }
  }
  CHECK(c3h::c3s_exist_of(0.0f, 0.0f) == 0);  // only a row without a voxel has exist 0
  CHECK(sizeof(c3h_packed_row) == sizeof(c3h::C3sPackedRow) && sizeof(c3h_packed_row) == 16);
}

int main() {
  check_ladders();
  check_exist();
  std::printf("head: %ld\nsequence: %ld\nvalue: %ld\npacked_rows ok\n", n_head, n_seq, n_value);
  return 0;
}
