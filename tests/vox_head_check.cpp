// vox_head_check.cpp -- the batched voxel head's host arithmetic (csrc/vosch_frames.h) on the
// host (its own main; built with -fsanitize=address,undefined by test_vox_head_cpu.py): the
// composite voxel key's widths, packing and order, the all-ones value behind every voxel of its
// frame, the per-frame status decision on every failure and on two at once, and the frame of a
// run ordinal with empty and failed frames at both ends and in the middle.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vosch_frames.h"

static long n_key = 0, n_status = 0, n_ordinal = 0;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static void check_key(int nf, int64_t nvox, int want_voxel_bits) {
  c3h::VfKey k{};
  CHECK(c3h::vh_key(nvox, nf, 1000, &k) == c3h::kVfOk);
  CHECK(k.cell_bits == want_voxel_bits && k.cell_bits == c3h::vf_bits((uint64_t)nvox));
  CHECK(k.frame_bits == c3h::vf_bits((uint64_t)(nf - 1)) && k.bits == k.cell_bits + k.frame_bits);
  CHECK(k.wide == 1 && k.bits <= 37);  // always 64-bit words
  const uint64_t none = c3h::vf_no_cell(k.cell_bits);
  CHECK(none >= (uint64_t)nvox);  // no voxel index (0 .. nvox - 1) is the all-ones value
  const int frames[] = {0, nf / 2, nf - 1};
  const int64_t voxels[] = {0, nvox / 2, nvox - 1};
  for (int f : frames)
    for (int64_t v : voxels) {
      const uint64_t key = c3h::vf_make_key(f, (uint64_t)v, k.cell_bits);
      CHECK(c3h::vf_key_frame(key, k.cell_bits) == f && c3h::vf_key_cell(key, k.cell_bits) == (uint64_t)v);
      CHECK(k.bits == 64 || (key >> k.bits) == 0);        // the sort's bits hold it
      const uint64_t dropped = c3h::vf_make_key(f, none, k.cell_bits);
      CHECK(key < dropped);  // behind every voxel of its frame,
      CHECK(k.bits == 64 || (dropped >> k.bits) == 0);
      if (f + 1 < nf) CHECK(dropped < c3h::vf_make_key(f + 1, 0, k.cell_bits));  // ahead of the next frame's first
      if (v > 0) CHECK(c3h::vf_make_key(f, (uint64_t)v - 1, k.cell_bits) < key);
      if (f > 0) CHECK(c3h::vf_make_key(f - 1, (uint64_t)nvox - 1, k.cell_bits) < c3h::vf_make_key(f, 0, k.cell_bits));
      ++n_key;
    }
}

static c3h::VhRec rec_of(int x0, int x1, int y0, int y1, int z0, int z1, unsigned long long nvalid, bool beyond) {
  c3h::VhRec r = c3h::vh_rec_init();
  if (nvalid) {
    r.mn[0] = x0, r.mx[0] = x1, r.mn[1] = y0, r.mx[1] = y1, r.mn[2] = z0, r.mx[2] = z1;
  }
  r.n_valid = nvalid;
  r.beyond = beyond ? 1u : 0u;
  return r;
}

static int decide(int64_t n, bool ptr, const c3h::VhRec& r, const c3h::VhCall& q, c3h::VhFrameGeom* g) {
  ++n_status;
  return c3h::vh_frame_decide(n, ptr, r, q, g);
}

static void check_status() {
  c3h::VhCall q{};
  q.leaf = 0.01f;
  q.radius = 0.02f;
  q.rsd_dist = 0.01f;
  q.subdiv = 4;
  q.offset[0] = 1, q.offset[1] = 0, q.offset[2] = 2;
  q.row_cap = 1000;
  c3h::VhFrameGeom g;
  const c3h::VhRec good = rec_of(-5, 14, 0, 19, 90, 109, 777, false);
  // a good frame: the geometry of the single-frame route
  CHECK(decide(1000, true, good, q, &g) == c3h::kVhGood);
  CHECK(g.div_b[0] == 20 && g.div_b[1] == 20 && g.div_b[2] == 20 && g.min_b[0] == -5 && g.max_b[2] == 109);
  CHECK(g.n_valid == 777 && g.nvox == 8000 && g.sb[0] == 5 && g.sb[1] == 5 && g.sb[2] == 5 && g.H == 125);
  {
    c3h::VfGrid want;
    CHECK(c3h::vf_nbr_grid(g.min_b, g.max_b, q.leaf, q.radius, &want) == c3h::kVfOk);
    CHECK(g.g.ncell == want.ncell && g.g.dim[0] == want.dim[0] && g.g.origin[2] == want.origin[2]);
    CHECK(g.g2.ncell == want.ncell && g.g2.cell == want.cell);  // no wide RSD radius: g2 = g
  }
  CHECK(c3h::vh_status(c3h::kVhGood) == 0);
  // every failure, alone
  CHECK(decide(-1, true, good, q, &g) == c3h::kVhArgs && c3h::vh_status(c3h::kVhArgs) == -1);
  CHECK(decide(5, false, good, q, &g) == c3h::kVhArgs);
  CHECK(decide(0, false, rec_of(0, 0, 0, 0, 0, 0, 0, false), q, &g) == c3h::kVhNoPoint);  // no pointer, no point: as n = 0
  CHECK(decide((int64_t)1 << 24, true, good, q, &g) == c3h::kVhPoints && c3h::vh_status(c3h::kVhPoints) == -5);
  CHECK(decide(((int64_t)1 << 24) - 1, true, good, q, &g) == c3h::kVhGood);
  CHECK(decide(10, true, rec_of(-5, 14, 0, 19, 90, 109, 9, true), q, &g) == c3h::kVhBeyond && c3h::vh_status(c3h::kVhBeyond) == -5);
  CHECK(decide(10, true, rec_of(0, 0, 0, 0, 0, 0, 0, false), q, &g) == c3h::kVhNoPoint && c3h::vh_status(c3h::kVhNoPoint) == -3);
  CHECK(decide(2, true, rec_of(0, 1300, 0, 1300, 50, 1350, 2, false), q, &g) == c3h::kVhVoxels && c3h::vh_status(c3h::kVhVoxels) == -5);
  {
    c3h::VhCall fine = q;
    fine.radius = 0.004f;  // 256 x 256 x 150 voxels: 643 x 643 x 378 search cells
    CHECK(decide(3000, true, rec_of(0, 255, 0, 255, 50, 199, 3000, false), fine, &g) == c3h::kVhCells);
    CHECK(c3h::vh_status(c3h::kVhCells) == -5);
    CHECK(decide(3000, true, rec_of(0, 255, 0, 255, 50, 199, 3000, false), q, &g) == c3h::kVhRows);  // 64 * 64 * 37 rows
    c3h::VhCall roomy = q;
    roomy.row_cap = 64 * 64 * 37;
    CHECK(decide(3000, true, rec_of(0, 255, 0, 255, 50, 199, 3000, false), roomy, &g) == c3h::kVhGood && g.H == 64 * 64 * 37);
    // the RSD's own grid (a wide leaf: leaf sqrt(3) / 2 > 4 x the normals radius)
    c3h::VhCall wide = roomy;
    wide.leaf = 0.1f;
    wide.radius = 0.02f;
    wide.rsd_dist = 0.0866f;
    wide.subdiv = 0;
    CHECK(c3h::vf_rsd_wide(wide.rsd_dist, wide.radius));
    CHECK(decide(30, true, rec_of(0, 4, 0, 4, 0, 4, 30, false), wide, &g) == c3h::kVhGood);
    CHECK(g.g2.cell == wide.rsd_dist && g.g.cell == wide.radius && g.g2.ncell != g.g.ncell && g.H == 1);
  }
  {
    c3h::VhCall tight = q;
    tight.row_cap = 124;
    CHECK(decide(1000, true, good, tight, &g) == c3h::kVhRows && c3h::vh_status(c3h::kVhRows) == -5);
    tight.row_cap = 125;
    CHECK(decide(1000, true, good, tight, &g) == c3h::kVhGood);
    // a frame without rows (the z offset reaches the grid's end) passes any row_cap
    tight.row_cap = 0;
    CHECK(decide(10, true, rec_of(0, 9, 0, 9, 0, 1, 10, false), tight, &g) == c3h::kVhGood && g.H == 0);
  }
  // two failures at once: the route's order decides
  CHECK(decide(-1, false, rec_of(0, 0, 0, 0, 0, 0, 0, true), q, &g) == c3h::kVhArgs);          // arguments before everything
  CHECK(decide((int64_t)1 << 25, true, rec_of(0, 0, 0, 0, 0, 0, 0, true), q, &g) == c3h::kVhPoints);
  CHECK(decide(10, true, rec_of(0, 0, 0, 0, 0, 0, 0, true), q, &g) == c3h::kVhBeyond);         // beyond before no valid point
  CHECK(decide(10, true, rec_of(0, 1300, 0, 1300, 50, 1350, 2, true), q, &g) == c3h::kVhBeyond);  // ... and before the product
  {
    c3h::VhCall fine = q;
    fine.radius = 0.0001f;
    fine.row_cap = 0;
    CHECK(decide(2, true, rec_of(0, 1300, 0, 1300, 50, 1350, 2, false), fine, &g) == c3h::kVhVoxels);  // product before cells, rows
    CHECK(decide(3000, true, rec_of(0, 255, 0, 255, 50, 199, 3000, false), fine, &g) == c3h::kVhCells);  // cells before rows
  }
}

// ordinals: frame f's runs are [pre[f], pre[f + 1]) of the batch's; a frame that failed or holds
// no voxel owns none
static void check_ordinals(const std::vector<int64_t>& nocc) {
  const int nf = (int)nocc.size();
  std::vector<int64_t> pre((size_t)nf + 1);
  const int64_t total = c3h::vf_prefix(nocc.data(), nf, pre.data());
  for (int64_t q = 0; q < total; ++q) {
    const int f = c3h::vf_frame_of(pre.data(), nf, q);
    CHECK(f >= 0 && f < nf && nocc[(size_t)f] > 0 && pre[(size_t)f] <= q && q < pre[(size_t)f + 1]);
    ++n_ordinal;
  }
}

int main() {
  const int frames[] = {1, 2, 33, 64};
  const struct {
    int64_t nvox;
    int bits;
  } voxels[] = {{1, 1}, {((int64_t)1 << 26) - 1, 26}, {(int64_t)1 << 26, 27}, {INT32_MAX, 31}};
  for (int nf : frames)
    for (const auto& v : voxels) check_key(nf, v.nvox, v.bits);
  c3h::VfKey k{};
  CHECK(c3h::vh_key(((int64_t)1 << 26) - 1, 64, 1, &k) == c3h::kVfOk && k.bits == 32);
  CHECK(c3h::vh_key((int64_t)1 << 26, 64, 1, &k) == c3h::kVfOk && k.bits == 33);
  CHECK(c3h::vh_key((int64_t)1 << 26, 33, 1, &k) == c3h::kVfOk && k.bits == 33);
  CHECK(c3h::vh_key(INT32_MAX, 1, 1, &k) == c3h::kVfOk && k.bits == 32);
  CHECK(c3h::vh_key(INT32_MAX, 2, 1, &k) == c3h::kVfOk && k.bits == 32);  // (frame_bits of one frame is 1 too)
  CHECK(c3h::vh_key(INT32_MAX, 64, 1, &k) == c3h::kVfOk && k.bits == 37 && k.wide == 1);
  CHECK(c3h::vh_key((int64_t)INT32_MAX + 1, 1, 1, &k) == c3h::kVfErrCells);
  CHECK(c3h::vh_key(1, 0, 1, &k) == c3h::kVfErrFrames && c3h::vh_key(1, 65, 1, &k) == c3h::kVfErrFrames);
  CHECK(c3h::vh_key(1, 1, c3h::kVfMaxPoints + 1, &k) == c3h::kVfErrPoints);
  check_status();
  check_ordinals({0, 0, 5, 0, 3, 0, 0, 1, 7, 0});
  check_ordinals({4, 0, 0, 2});
  check_ordinals({0, 9});
  check_ordinals({9, 0});
  check_ordinals({1});
  check_ordinals({0, 0, 0});
  {
    std::vector<int64_t> many(64, 0);
    for (int f = 0; f < 64; ++f) many[(size_t)f] = (f % 3 == 1) ? 0 : f + 1;
    many[0] = many[63] = 0;
    check_ordinals(many);
  }
  std::printf("key: %ld\nstatus: %ld\nordinal: %ld\nvox_head ok\n", n_key, n_status, n_ordinal);
  return 0;
}
