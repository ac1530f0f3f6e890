// c3_sparse_check.cpp -- the host arithmetic of the sparse batched C3-HLAC-981 (csrc/c3_sparse.h)
// on the host (its own main; built with -fsanitize=address,undefined by test_c3_sparse_cpu.py):
// the row key's packing and order with the "none" value last, the chunk plan of a group, the
// inverse bin table against the closed form of the layout, and the subdivision of an acting cell
// at its skip and drop edges.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "c3_sparse.h"

static long n_key = 0, n_plan = 0, n_bin = 0, n_sub = 0;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

// nf frames of `rows` rows each (frame 1 of a batch of several: none)
static void check_key(int nf, int64_t rows) {
  std::vector<int64_t> hpre((size_t)nf + 1, 0);
  for (int f = 0; f < nf; ++f) hpre[(size_t)f + 1] = hpre[(size_t)f] + (nf > 1 && f == 1 ? 0 : rows);
  const int64_t htot = hpre[(size_t)nf];
  const int bits = c3h::c3s_key_bits(htot);
  const uint64_t none = c3h::c3s_none(htot);
  CHECK(bits >= 1 && bits <= 64 && (bits == 64 || (none >> bits) == 0));  // the sort's bits hold every value
  uint64_t last = 0;
  bool first = true;
  for (int f = 0; f < nf; ++f) {
    const int64_t H = hpre[(size_t)f + 1] - hpre[(size_t)f];
    const int64_t subs[] = {0, H / 2, H - 1};
    for (int64_t h : subs) {
      if (h < 0 || h >= H) continue;
      const uint64_t key = c3h::c3s_key(hpre.data(), f, h);
      CHECK(key < none);                                             // "none" sorts last
      CHECK(c3h::vf_frame_of(hpre.data(), nf, (int64_t)key) == f);   // the key is the row's batch ordinal:
      CHECK((int64_t)key - hpre[(size_t)f] == h);                    // its frame and subdivision come back
      CHECK(first || key >= last);                                   // ordered by (frame, subdivision)
      if (h > 0) CHECK(c3h::c3s_key(hpre.data(), f, h - 1) < key);
      last = key;
      first = false;
      ++n_key;
    }
  }
}

static void check_plan(int64_t L, int64_t want_chunks) {
  CHECK(c3h::c3s_chunks(L) == want_chunks);
  int64_t sum = 0;
  for (int64_t i = 0; i < want_chunks; ++i) {
    const int64_t n = c3h::c3s_chunk_len(L, i);
    CHECK(n >= 1 && n <= c3h::kC3sChunk);
    CHECK(i + 1 == want_chunks || n == c3h::kC3sChunk);  // only the last may be short
    sum += n;
    ++n_plan;
  }
  CHECK(sum == L && c3h::c3s_chunk_len(L, want_chunks) == 0);
  // the host's bounds hold for a batch that is this group alone, and with a row per voxel
  CHECK(want_chunks <= c3h::c3s_chunk_cap(L, 1) || L == 0);
  CHECK((want_chunks > 1 ? 1 : 0) <= c3h::c3s_multi_cap(L));
  CHECK(c3h::c3s_chunk_cap(L, L) >= L);
  ++n_plan;
}

static void check_bins() {
  const c3h::C3sTable tab = c3h::c3s_make_table();
  std::set<int> seen;
  auto claim = [&](int bin, int pos, int fa, int fb) {
    CHECK(bin >= 0 && bin < c3h::kC3sBins && seen.insert(bin).second);
    const c3h::C3sBin d = c3h::c3s_bin_desc(bin);
    CHECK(d.pos == pos && d.fa == fa && d.fb == fb);
    const uint32_t w = tab.v[bin];
    CHECK((int)(w & 15u) == pos && (int)(w >> 4 & 63u) == c3h::c3s_field_shift(fa) &&
          (int)(w >> 10 & 63u) == c3h::c3s_field_shift(fb));
    CHECK(((w >> 16 & 1u) != 0) == (fa < 6) && ((w >> 17 & 1u) != 0) == (fb < 6) && (w >> 18 & 1u) == 1u);
    ++n_bin;
  };
  const int B = c3h::kC3sFieldBeta, One = c3h::kC3sFieldOne;
  for (int c = 0; c < 6; ++c) {  // zero order, then (k, c, n), then the centre's own pairs
    claim(c, 0, c, One);
    claim(495 + c, 0, B + c, One);
    for (int n = 0; n < 6; ++n)
      for (int k = 0; k < 13; ++k) {
        claim(c3h::c3s_bin981(k, c, n), 1 + k, c, n);
        claim(495 + c3h::c3s_bin981(k, c, n), 1 + k, B + c, B + n);
      }
    for (int n = c; n < 6; ++n) claim(474 + c3h::c3s_tri6(c, n), 0, c, n);  // the auto-product triangle
  }
  for (int c = 0; c < 4; ++c)  // the twelve binarised pairs of different colour channels
    for (int n = (c < 2 ? 2 : 4); n < 6; ++n)
      claim(c < 2 ? 969 + 4 * c + (n - 2) : 977 + 2 * (c - 2) + (n - 4), 0, B + c, B + n);
  CHECK((int)seen.size() == c3h::kC3sBins && *seen.begin() == 0 && *seen.rbegin() == 980);  // a bijection onto 0 .. 980
  for (int i = c3h::kC3sBins; i < c3h::kC3sBlock * c3h::kC3sBinsPerThread; ++i) CHECK(tab.v[i] == 0);
  // the fields of a staged word do not overlap and the constant is the word's top bit
  uint64_t used = 0;
  for (int f = 0; f <= One; ++f) {
    const uint64_t m = (uint64_t)c3h::c3s_field_mask(f) << c3h::c3s_field_shift(f);
    CHECK((used & m) == 0);
    used |= m;
  }
  CHECK(c3h::c3s_field_shift(One) == 63);
  for (int k = 0; k < 13; ++k) {  // 13 distinct neighbours, none the centre, all in the lower half
    int r[3];
    c3h::c3s_rel(k, r);
    CHECK(r[0] >= -1 && r[0] <= 1 && r[1] >= -1 && r[1] <= 1 && r[2] >= -1 && r[2] <= 0);
    CHECK(r[2] < 0 || r[1] < 0 || (r[1] == 0 && r[0] < 0));
  }
}

static void check_subdivision() {
  const int off[3] = {1, 0, 2}, sb[3] = {3, 2, 2};
  const float inv_s = 1.0 / 4;
  auto sub = [&](int x, int y, int z, int hist1) {
    const int a[3] = {x, y, z};
    ++n_sub;
    return c3h::c3s_subdivision(a, off, sb, inv_s, hist1);
  };
  CHECK(sub(1, 0, 2, 0) == 0);                      // the first cell at the offset
  CHECK(sub(0, 0, 2, 0) == -1 && sub(1, -1, 2, 0) == -1 && sub(1, 0, 1, 0) == -1);  // below it on one axis: skipped
  CHECK(sub(4, 3, 5, 0) == 0 && sub(5, 3, 5, 0) == 1 && sub(4, 4, 5, 0) == 3 && sub(4, 3, 6, 0) == 6);
  CHECK(sub(12, 7, 9, 0) == 2 + 3 * (1 + 2 * 1));   // the last cell of the last subdivision
  CHECK(sub(13, 7, 9, 0) == -1 && sub(12, 8, 9, 0) == -1 && sub(12, 7, 10, 0) == -1);  // one past it: dropped
  CHECK(sub(-5, 100, -1, 1) == 0);                  // one row: histogram 0 wherever the cell lies
  const int off0[3] = {0, 0, 0}, sb1[3] = {2, 1, 1};  // subdivision 10 of a 12-cell axis
  for (int x = -1; x <= 20; ++x) {
    const int a[3] = {x, 0, 0};
    const int64_t want = x < 0 || x >= 20 ? -1 : x / 10;
    CHECK(c3h::c3s_subdivision(a, off0, sb1, (float)(1.0 / 10), 0) == want);
    ++n_sub;
  }
}

int main() {
  const int64_t rows[] = {1, 2, 1000, ((int64_t)1 << 31) - 1};  // up to the largest row count of a frame
  for (int nf : {1, 2, 64})
    for (int64_t r : rows) check_key(nf, r);
  check_plan(0, 0);
  check_plan(1, 1);
  check_plan(c3h::kC3sChunk, 1);
  check_plan(c3h::kC3sChunk + 1, 2);
  check_plan(90000, (90000 + c3h::kC3sChunk - 1) / c3h::kC3sChunk);
  check_bins();
  check_subdivision();
  std::printf("key: %ld\nplan: %ld\nbin: %ld\nsub: %ld\nc3_sparse ok\n", n_key, n_plan, n_bin, n_sub);
  return 0;
}
