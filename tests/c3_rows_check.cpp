// c3_rows_check.cpp -- the host arithmetic of the sparse C3-HLAC-117 (csrc/c3_sparse.h) on the host
// (its own main; built with -fsanitize=address,undefined by test_c3_rows_cpu.py): the inverse
// 117-bin table as a surjection of the (position, field, field) terms of the 981 layout onto bins
// 0 .. 116 that agrees with fold117's closed form for every (k, c, n), with the auto-product
// triangle and with the twelve binarised pairs; the packing of a voxel's record; the u32 bound of a
// chunk's sums.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "c3_sparse.h"

static long n_term = 0, n_bin = 0, n_field = 0;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

typedef std::tuple<int, int, int> Term;  // (position, centre field, position's field) in the 981 numbering

// fold117 (c3hlac_dev.h), written out again: the 981 bins that 117-bin i adds up
static std::vector<int> fold117_bins(int i) {
  std::vector<int> out;
  if (i < 6) out.push_back(i);
  else if (i < 42) {
    const int c = (i - 6) / 6, n = (i - 6) % 6;
    for (int k = 0; k < 13; ++k) out.push_back(c3h::c3s_bin981(k, c, n));
  } else if (i < 63) out.push_back(474 + (i - 42));
  else if (i < 69) out.push_back(495 + (i - 63));
  else if (i < 105) {
    const int c = (i - 69) / 6, n = (i - 69) % 6;
    for (int k = 0; k < 13; ++k) out.push_back(495 + c3h::c3s_bin981(k, c, n));
  } else out.push_back(969 + (i - 105));
  return out;
}

// the 981 terms a 117 descriptor stands for: field numbering 0 one, 1 .. 6 a, 7 .. 12 beta,
// 13 .. 18 N (the 13 neighbours' a), 19 .. 24 B (the 13 neighbours' beta)
static std::set<Term> expand(const c3h::C3s117Bin& d) {
  std::set<Term> out;
  const int B = c3h::kC3sFieldBeta, One = c3h::kC3sFieldOne;
  auto centre = [&](int f) { return f < 7 ? f - 1 : B + (f - 7); };  // a 117 field 1 .. 12 as a 981 field
  if (d.fx == 0) {
    CHECK(d.fy >= 1 && d.fy <= 12);
    out.insert(Term(0, centre(d.fy), One));
  } else if (d.fy >= 13) {
    CHECK(d.fx >= 1 && d.fx <= 12);
    const bool bin = d.fy >= 19;
    CHECK(bin == (d.fx >= 7));  // colour with colour, binarised with binarised
    for (int k = 0; k < 13; ++k) out.insert(Term(1 + k, centre(d.fx), (bin ? B : 0) + (d.fy - (bin ? 19 : 13))));
  } else {
    CHECK(d.fx >= 1 && d.fx <= 12 && d.fy >= 1 && d.fy <= 12 && (d.fx >= 7) == (d.fy >= 7));
    out.insert(Term(0, centre(d.fx), centre(d.fy)));
  }
  return out;
}

static void check_bins() {
  const c3h::C3s117Table tab = c3h::c3s117_make_table();
  std::set<Term> all;
  std::set<int> bins981;
  for (int i = 0; i < c3h::kC3s117Bins; ++i) {
    const c3h::C3s117Bin d = c3h::c3s117_bin_desc(i);
    const std::set<Term> mine = expand(d);
    std::set<Term> want;
    for (int j : fold117_bins(i)) {
      CHECK(j >= 0 && j < c3h::kC3sBins && bins981.insert(j).second);  // every 981 bin folds into one 117 bin
      CHECK(c3h::c3s117_of_981(j) == i);
      const c3h::C3sBin b = c3h::c3s_bin_desc(j);
      CHECK(want.insert(Term(b.pos, b.fa, b.fb)).second);
      ++n_term;
    }
    CHECK(mine == want);  // the closed form, for every (k, c, n), the triangle and the pairs
    for (const Term& t : mine) CHECK(all.insert(t).second);
    // the packed word
    const uint32_t w = tab.v[i];
    CHECK((int)(w & 7u) == c3h::c3s117_field_word(d.fx) && (int)(w >> 3 & 31u) == c3h::c3s117_field_shift(d.fx) &&
          (int)(w >> 8 & 31u) == c3h::c3s117_field_bits(d.fx));
    CHECK((int)(w >> 13 & 7u) == c3h::c3s117_field_word(d.fy) && (int)(w >> 16 & 31u) == c3h::c3s117_field_shift(d.fy) &&
          (int)(w >> 21 & 31u) == c3h::c3s117_field_bits(d.fy) && (w >> 26) == 1u);
    ++n_bin;
  }
  CHECK((int)bins981.size() == c3h::kC3sBins && (int)all.size() == c3h::kC3sBins);  // onto: no term left out
  for (int i = c3h::kC3s117Bins; i < 128; ++i) CHECK(tab.v[i] == 0);
  // explicit spot checks of the layout: (c, n) of the first-order bins, the triangle, the pairs
  for (int c = 0; c < 6; ++c)
    for (int n = 0; n < 6; ++n) {
      const c3h::C3s117Bin a = c3h::c3s117_bin_desc(6 + 6 * c + n), b = c3h::c3s117_bin_desc(69 + 6 * c + n);
      CHECK(a.fx == 1 + c && a.fy == 13 + n && b.fx == 7 + c && b.fy == 19 + n);
      if (n >= c) {
        const c3h::C3s117Bin t = c3h::c3s117_bin_desc(42 + c3h::c3s_tri6(c, n));
        CHECK(t.fx == 1 + c && t.fy == 1 + n);
      }
    }
  for (int c = 0; c < 4; ++c)
    for (int n = (c < 2 ? 2 : 4); n < 6; ++n) {
      const c3h::C3s117Bin p = c3h::c3s117_bin_desc(c < 2 ? 105 + 4 * c + (n - 2) : 113 + 2 * (c - 2) + (n - 4));
      CHECK(p.fx == 7 + c && p.fy == 7 + n);
    }
}

static void check_record_and_bound() {
  // the fields of a record do not overlap, lie in their word, and hold their largest value
  uint32_t used[c3h::kC3s117Words] = {0, 0, 0, 0, 0, 0};
  const uint64_t maxv[5] = {1, 255, 1, 13 * 255, 13};
  for (int f = 0; f < c3h::kC3s117Fields; ++f) {
    const int w = c3h::c3s117_field_word(f), s = c3h::c3s117_field_shift(f), b = c3h::c3s117_field_bits(f);
    CHECK(w >= 0 && w < c3h::kC3s117Words && s >= 0 && b >= 1 && s + b <= 32);
    const uint32_t m = (uint32_t)((((uint64_t)1 << b) - 1) << s);
    CHECK((used[w] & m) == 0);
    used[w] |= m;
    const int kind = f == 0 ? 0 : f < 7 ? 1 : f < 13 ? 2 : f < 19 ? 3 : 4;
    CHECK(maxv[kind] < ((uint64_t)1 << b));
    ++n_field;
  }
  // words 0 and 1 are the two halves of the 981 pass's staged word: the centre needs no repacking
  for (int c = 0; c < 6; ++c) {
    CHECK(32 * c3h::c3s117_field_word(1 + c) + c3h::c3s117_field_shift(1 + c) == c3h::c3s_field_shift(c));
    CHECK(32 * c3h::c3s117_field_word(7 + c) + c3h::c3s117_field_shift(7 + c) == c3h::c3s_field_shift(c3h::kC3sFieldBeta + c));
  }
  CHECK(32 * c3h::c3s117_field_word(0) + c3h::c3s117_field_shift(0) == c3h::c3s_field_shift(c3h::kC3sFieldOne));
  // the u32 bound of a chunk: the largest product of any bin's two fields, over a chunk's voxels
  uint64_t worst = 0;
  for (int i = 0; i < c3h::kC3s117Bins; ++i) {
    const c3h::C3s117Bin d = c3h::c3s117_bin_desc(i);
    auto top = [&](int f) { return maxv[f == 0 ? 0 : f < 7 ? 1 : f < 13 ? 2 : f < 19 ? 3 : 4]; };
    worst = std::max(worst, top(d.fx) * top(d.fy));
  }
  CHECK(worst == (uint64_t)13 * 65025);
  CHECK(worst * c3h::kC3sChunk < ((uint64_t)1 << 32));
  CHECK(c3h::kC3sChunk != 1024 || worst * c3h::kC3sChunk == 865612800ull);  // 8.66e8
  CHECK(worst * 8000 > ((uint64_t)1 << 32));  // a row of 8,000 white voxels needs the 64-bit slots
  CHECK(c3h::kC3sChunk % c3h::kC3s117Slice == 0 && c3h::kC3s117Slice == 64 && c3h::kC3s117Waves == 4);
}

int main() {
  check_bins();
  check_record_and_bound();
  std::printf("term: %ld\nbin: %ld\nfield: %ld\nc3_rows ok\n", n_term, n_bin, n_field);
  return 0;
}
