// vosch_frames_check.cpp -- csrc/vosch_frames.h on the host (its own main; built with
// -fsanitize=address,undefined by test_vosch_frames_cpu.py): the prefixes and the frame of an
// index at every boundary (empty frames in the middle and at both ends), each frame's search
// grid against a literal transcription of the single-frame arithmetic it replaced, the composite key widths, its
// packing and the capacity errors, the subdivision counts against grsd_frames' statements.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vosch_frames.h"

static long n_prefix = 0, n_grid = 0, n_key = 0, n_sub = 0;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static void check_prefix(const std::vector<int64_t>& n) {
  const int nf = (int)n.size();
  std::vector<int64_t> pre((size_t)nf + 1, -1);
  const int64_t total = c3h::vf_prefix(n.data(), nf, pre.data());
  int64_t sum = 0;
  for (int f = 0; f < nf; ++f) {
    CHECK(pre[(size_t)f] == sum);
    sum += n[(size_t)f];
  }
  CHECK(total == sum && pre[(size_t)nf] == sum);
  // every index near every boundary (all of them when the total is small): the linear scan
  for (int f = 0; f < nf; ++f)
    for (int64_t d = -2; d <= 2; ++d)
      for (int side = 0; side < 2; ++side) {
        const int64_t i = (side ? pre[(size_t)f + 1] : pre[(size_t)f]) + d;
        if (i < 0 || i >= total) continue;
        int want = -1;
        for (int g = 0; g < nf; ++g)
          if (pre[(size_t)g] <= i && i < pre[(size_t)g + 1]) want = g;
        CHECK(want >= 0 && n[(size_t)want] > 0);
        CHECK(c3h::vf_frame_of(pre.data(), nf, i) == want);
        ++n_prefix;
      }
  if (total <= 4096)
    for (int64_t i = 0; i < total; ++i) {
      const int f = c3h::vf_frame_of(pre.data(), nf, i);
      CHECK(f >= 0 && f < nf && pre[(size_t)f] <= i && i < pre[(size_t)f + 1]);
      ++n_prefix;
    }
}

// the former nbr_grid() of capi.hip, statement by statement
static void ref_nbr_grid(const int32_t min_b[3], const int32_t max_b[3], float leaf, float cell, float origin[3], int dim[3],
                         float* inv_cell, bool* too_many) {
  *inv_cell = 1.0f / cell;
  for (int ax = 0; ax < 3; ++ax) {
    const double lo = (double)min_b[ax] * leaf, hi = (double)(max_b[ax] + 1) * leaf;
    origin[ax] = (float)(lo - cell);
    dim[ax] = (int)std::ceil((hi - lo) / cell) + 3;
  }
  const int64_t ncell = (int64_t)dim[0] * dim[1] * dim[2];
  *too_many = ncell > ((int64_t)1 << 27);
}

static void check_grid(const int32_t min_b[3], const int32_t max_b[3], float leaf, float cell) {
  c3h::VfGrid g;
  std::memset(&g, 0, sizeof(g));
  const int rc = c3h::vf_nbr_grid(min_b, max_b, leaf, cell, &g);
  float origin[3], inv;
  int dim[3];
  bool too_many;
  ref_nbr_grid(min_b, max_b, leaf, cell, origin, dim, &inv, &too_many);
  CHECK((rc == c3h::kVfErrCells) == too_many && (rc == c3h::kVfOk) == !too_many);
  CHECK(std::memcmp(&g.inv_cell, &inv, 4) == 0 && g.cell == cell);
  for (int a = 0; a < 3; ++a) CHECK(std::memcmp(&g.origin[a], &origin[a], 4) == 0 && g.dim[a] == dim[a]);
  CHECK(g.ncell == (int64_t)dim[0] * dim[1] * dim[2]);
  ++n_grid;
}

static void check_keys() {
  c3h::VfKey k;
  // widths: cell_bits holds the value max_cells (the no-cell mark), frame_bits the last frame
  const int64_t cells[] = {1, 2, 3, 4, 255, 256, 257, 65535, 65536, (1 << 20) + 1, ((int64_t)1 << 26) - 1,
                           (int64_t)1 << 26, ((int64_t)1 << 27) - 1, (int64_t)1 << 27};
  for (int64_t mc : cells)
    for (int nf = 1; nf <= c3h::kVfMaxFrames; ++nf) {
      CHECK(c3h::vf_key(mc, nf, 1000, &k) == c3h::kVfOk);
      CHECK(((uint64_t)1 << k.cell_bits) > (uint64_t)mc && (k.cell_bits == 1 || ((uint64_t)1 << (k.cell_bits - 1)) <= (uint64_t)mc));
      CHECK(((uint64_t)1 << k.frame_bits) >= (uint64_t)nf && (k.frame_bits == 1 || ((uint64_t)1 << (k.frame_bits - 1)) < (uint64_t)nf));
      CHECK(k.bits == k.cell_bits + k.frame_bits && k.bits <= 64 && k.wide == (k.bits > 32));
      if (nf == 1) CHECK(k.frame_bits == 1 && k.bits <= 29 && !k.wide);  // a single frame: 32-bit keys at every grid size
      const uint64_t none = c3h::vf_no_cell(k.cell_bits);
      CHECK(none >= (uint64_t)mc);  // above every real cell index 0 .. mc - 1
      // packing round trip, and the order: frame first, then cell, the no-cell mark last in its frame
      const uint64_t cs[] = {0, (uint64_t)mc - 1, none};
      uint64_t prev = 0;
      bool first = true;
      std::vector<int> fs = {0};
      if (nf / 2 > 0) fs.push_back(nf / 2);
      if (nf - 1 > nf / 2) fs.push_back(nf - 1);
      for (int f : fs)
        for (uint64_t c : cs) {
          const uint64_t key = c3h::vf_make_key(f, c, k.cell_bits);
          CHECK(c3h::vf_key_frame(key, k.cell_bits) == f && c3h::vf_key_cell(key, k.cell_bits) == c);
          CHECK(k.bits == 64 || (key >> k.bits) == 0);
          if (!k.wide) CHECK((uint64_t)(uint32_t)key == key);
          CHECK(first || key >= prev);
          prev = key;
          first = false;
          ++n_key;
        }
    }
  CHECK(c3h::vf_bits(0) == 1 && c3h::vf_bits(1) == 1 && c3h::vf_bits(2) == 2 && c3h::vf_bits(63) == 6 && c3h::vf_bits(64) == 7);
  CHECK(c3h::vf_bits(~(uint64_t)0) == 64);
  // capacity errors
  CHECK(c3h::vf_key(((int64_t)1 << 27) + 1, 4, 10, &k) == c3h::kVfErrCells);
  CHECK(c3h::vf_key(-1, 4, 10, &k) == c3h::kVfErrCells);
  CHECK(c3h::vf_key(100, 0, 10, &k) == c3h::kVfErrFrames);
  CHECK(c3h::vf_key(100, c3h::kVfMaxFrames + 1, 10, &k) == c3h::kVfErrFrames);
  CHECK(c3h::vf_key(100, 4, (int64_t)1 << 32, &k) == c3h::kVfErrPoints);
  CHECK(c3h::vf_key(100, 4, ((int64_t)1 << 32) - 1, &k) == c3h::kVfOk);
  CHECK(c3h::vf_key(100, 4, -1, &k) == c3h::kVfErrPoints);
  // the largest batch: 2^27 cells, 64 frames -> 28 + 6 bits, wide
  CHECK(c3h::vf_key((int64_t)1 << 27, 64, 1, &k) == c3h::kVfOk && k.cell_bits == 28 && k.frame_bits == 6 && k.wide == 1);
  CHECK(c3h::vf_key(((int64_t)1 << 26) - 1, 64, 1, &k) == c3h::kVfOk && k.bits == 32 && k.wide == 0);
}

// grsd_frames' subdivision statements (capi.hip before this header; grsd_colorCHLAC_tools.hpp:150-162)
static int64_t ref_subdiv(const int32_t div[3], int32_t subdiv, const int32_t off[3], int32_t sb[3], float* inv_s_out) {
  int64_t H = 1;
  float inv_s = 0.0f;
  sb[0] = sb[1] = sb[2] = 0;
  *inv_s_out = 0.0f;
  if (subdiv > 0) {
    inv_s = 1.0 / subdiv;
    *inv_s_out = inv_s;
    if (div[0] <= off[0] || div[1] <= off[1] || div[2] <= off[2]) return 0;
    for (int a = 0; a < 3; ++a) sb[a] = (int)ceilf((div[a] - off[a]) * inv_s);
    H = (int64_t)sb[0] * sb[1] * sb[2];
  } else if (subdiv < 0) {
    return 0;
  } else {
    sb[0] = sb[1] = sb[2] = 1;
  }
  return H;
}

int main() {
  check_prefix({5});
  check_prefix({0});
  check_prefix({0, 0, 0});
  check_prefix({0, 7, 0, 0, 3, 1, 0});         // empty at both ends and in the middle
  check_prefix({1, 0, 1, 0, 1});
  check_prefix({3, 0, 0, 0, 0, 0, 0, 2});
  check_prefix({0, 0, 9});
  check_prefix({9, 0, 0});
  check_prefix(std::vector<int64_t>(64, 1));
  check_prefix(std::vector<int64_t>(64, 0));
  {
    std::vector<int64_t> n(64);
    for (int f = 0; f < 64; ++f) n[(size_t)f] = f % 5 == 0 ? 0 : (int64_t)(f * 37 % 11);
    check_prefix(n);
    for (int f = 0; f < 64; ++f) n[(size_t)f] = f % 3 == 1 ? 0 : ((int64_t)1 << 25) + f;  // beyond int32 totals
    check_prefix(n);
    n.assign(3, ((int64_t)1 << 32) / 3);
    check_prefix(n);
  }

  const float leaves[] = {0.01f, 0.02f, 0.005f, 0.1f, 0.0123f};
  const float cells[] = {0.02f, 0.04f, 0.01f, 0.0866025f, 0.5f, 0.001f};
  const int32_t boxes[][6] = {{0, 0, 0, 0, 0, 0},       {-12, 3, 80, 40, 60, 140},   {-50, -50, 50, 49, 49, 149},
                              {100, -7, 0, 100, 30, 0}, {-1048576, 0, 0, -1048000, 5, 5}, {0, 0, 0, 2047, 2047, 63},
                              {5, 5, 5, 5, 5, 5},       {-3, -2, -1, 3, 2, 1}};
  for (float leaf : leaves)
    for (float cell : cells)
      for (const auto& b : boxes) check_grid(b, b + 3, leaf, cell);
  {  // more than 2^27 cells
    const int32_t lo[3] = {0, 0, 0}, hi[3] = {5999, 5999, 5999};
    c3h::VfGrid g;
    CHECK(c3h::vf_nbr_grid(lo, hi, 0.01f, 0.02f, &g) == c3h::kVfErrCells);
    check_grid(lo, hi, 0.01f, 0.02f);
  }
  // reach: max(1, (int)ceilf(radius * inv_cell))
  for (float r : {0.02f, 0.04f, 0.013f, 0.1f, 0.0866025f})
    for (float c : {0.02f, 0.04f, 0.013f, 0.1f, 0.0866025f, 0.005f}) {
      const float inv = 1.0f / c;
      const int want = std::max(1, (int)ceilf(r * inv));
      CHECK(c3h::vf_reach(r, inv) == want);
      if (r == c) CHECK(want <= 2);
      ++n_grid;
    }

  check_keys();

  for (int32_t subdiv : {-1, 0, 1, 3, 4, 10, 70})
    for (int32_t d0 : {1, 2, 4, 5, 17, 70, 71})
      for (int32_t o : {0, 1, 2, 5, 17}) {
        const int32_t div[3] = {d0, d0 + 3, 2 * d0}, off[3] = {o, 0, o / 2};
        int32_t sa[3], sb[3];
        float ia, ib;
        const int64_t Ha = c3h::vf_subdivisions(div, subdiv, off, sa, &ia);
        const int64_t Hb = ref_subdiv(div, subdiv, off, sb, &ib);
        CHECK(Ha == Hb && std::memcmp(sa, sb, sizeof(sa)) == 0 && std::memcmp(&ia, &ib, 4) == 0);
        ++n_sub;
      }

  std::printf("prefix: %ld\ngrid: %ld\nkey: %ld\nsubdiv: %ld\nvosch_frames ok\n", n_prefix, n_grid, n_key, n_sub);
  return 0;
}
