// Host check of the feature-rows front's index arithmetic (mapping-private_amd/csrc/
// feat_rows.h), built with -fsanitize=address,undefined and run by test_feature_frames_cpu.py.
//   - the three exist rules against literal transcriptions of the reference's statements
//     (search_c3_hlac.h:60-61, search_new.h:41-43 and 69-74), on values where the float / int
//     order of the operations decides the result;
//   - the canvas row <-> frame row mapping, both ways, on the shapes of the GPU tests;
//   - the row-block and alignment plan for dim 21, 22, 137 and 981 at every word misalignment
//     of the frame's base: every element of every span is covered exactly once, vector loads
//     and their LDS slots are 16-byte aligned, and the stage holds the span.
// Prints one line per part; exit status 0 iff all hold.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "feat_rows.h"

using namespace c3h;

static int g_fail = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (g_fail < 20) {                        \
        fprintf(stderr, "FAIL %s: ", #cond);    \
        fprintf(stderr, __VA_ARGS__);           \
        fprintf(stderr, "\n");                  \
      }                                         \
      ++g_fail;                                 \
    }                                           \
  } while (0)

// ---- the reference's statements, as written there (feature: float rows, exist_voxel_num: int)
static int ref_c3hlac(const float* feature) {  // search_c3_hlac.h:60-61
  int exist_voxel_num;
  exist_voxel_num = (feature[0] + feature[1]) * 2 + 0.001;
  return exist_voxel_num;
}
static int ref_vosch(const float* feature) {  // search_new.h:41-43
  int exist_voxel_num;
  exist_voxel_num = (feature[20] + feature[21]) * 2 + 0.001;
  return exist_voxel_num;
}
static int ref_grsd(const float* feature) {  // search_new.h:69-74
  int exist_voxel_num = 0;
  for (int j = 0; j < 20; j++) exist_voxel_num += feature[j];
  exist_voxel_num /= 26;
  return exist_voxel_num;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int check_rules() {
  int n = 0;
  std::vector<float> f(137);
  // pairs where float addition rounds (2^24 + 1 is no float; the double sum would differ),
  // where + 0.001 crosses an integer, and plain counts
  const float pairs[][2] = {{16777216.0f, 1.0f}, {16777216.0f, 3.0f}, {8388608.5f, 0.5f}, {0.4995f, 0.0f},
                            {0.49951f, 0.0f}, {0.25f, 0.24975f}, {1e-4f, 3e-4f}, {0.0f, 0.0f}, {-0.0f, 0.0f},
                            {12.0f, 30.5f}, {1000000.0f, 0.03f}, {3.9996f, 0.0f}, {0.1f, 0.2f}, {33554432.0f, 2.0f}};
  for (const auto& p : pairs)
    for (int rule = 0; rule < 2; ++rule) {
      for (auto& v : f) v = 7.0f;
      const int i0 = rule ? 20 : 0;
      f[i0] = p[0];
      f[i0 + 1] = p[1];
      const int want = rule ? ref_vosch(f.data()) : ref_c3hlac(f.data());
      CHECK(fr_exist_rule(f.data(), rule) == want, "rule %d (%g, %g): %d != %d", rule, p[0], p[1],
            fr_exist_rule(f.data(), rule), want);
      ++n;
    }
  // GRSD: the int is truncated after every float add (20 x 1.6 gives 20, not 32), and large
  // counts where (float)int + float rounds
  for (int t = 0; t < 2000; ++t) {
    uint32_t s = 12345u + 977u * t;
    for (int j = 0; j < 21; ++j) {
      const uint32_t r = lcg(s) >> 8;
      switch (t % 5) {
        case 0: f[j] = 1.6f; break;
        case 1: f[j] = (float)(r % 60); break;
        case 2: f[j] = (float)(r % 2000) * 0.37f; break;
        case 3: f[j] = j == 0 ? 16777216.0f : (float)(r % 7) * 0.5f + 1.0f; break;
        default: f[j] = (float)(r % 3) * 0.999f; break;
      }
    }
    const int want = ref_grsd(f.data());
    CHECK(fr_exist_rule(f.data(), 2) == want, "grsd case %d: %d != %d", t, fr_exist_rule(f.data(), 2), want);
    ++n;
  }
  for (auto& v : f) v = 1.6f;
  CHECK(fr_exist_rule(f.data(), 2) == 20 / 26, "per-add truncation");
  CHECK(fr_exist_min_dim(0) == 2 && fr_exist_min_dim(1) == 22 && fr_exist_min_dim(2) == 20, "dim minimums");
  return n;
}

static int64_t check_mapping() {
  const int canvases[][3] = {{16, 16, 16}, {26, 26, 26}, {7, 5, 3}, {1, 1, 1}};
  const int frames[][3] = {{16, 16, 16}, {13, 16, 9}, {1, 16, 16}, {16, 1, 16}, {5, 3, 2}, {7, 5, 3}, {1, 1, 1},
                           {0, 16, 16}, {26, 26, 26}, {25, 26, 1}};
  int64_t n = 0;
  for (const auto& cb : canvases)
    for (const auto& sb : frames) {
      if (sb[0] > cb[0] || sb[1] > cb[1] || sb[2] > cb[2]) continue;
      const int64_t Hc = (int64_t)cb[0] * cb[1] * cb[2], Hf = (int64_t)sb[0] * sb[1] * sb[2];
      std::vector<int> hit((size_t)Hf, 0);
      int64_t inside = 0;
      for (int64_t c = 0; c < Hc; ++c) {
        const int x = (int)(c % cb[0]), y = (int)(c / cb[0] % cb[1]), z = (int)(c / cb[0] / cb[1]);
        const bool in = x < sb[0] && y < sb[1] && z < sb[2];
        const int64_t h = fr_canvas_to_frame(c, cb, sb);
        CHECK((h >= 0) == in, "canvas row %lld of (%d %d %d) in (%d %d %d)", (long long)c, sb[0], sb[1], sb[2], cb[0],
              cb[1], cb[2]);
        if (h < 0) continue;
        CHECK(h < Hf, "frame row in range");
        if (h >= Hf) continue;
        CHECK(h == x + (int64_t)sb[0] * (y + (int64_t)sb[1] * z), "frame row of (x, y, z)");
        CHECK(fr_frame_to_canvas(h, cb, sb) == c, "round trip of canvas row %lld", (long long)c);
        hit[(size_t)h]++;
        ++inside;
      }
      CHECK(inside == Hf, "%lld canvas rows inside, %lld frame rows", (long long)inside, (long long)Hf);
      for (int64_t h = 0; h < Hf; ++h) {
        CHECK(hit[(size_t)h] == 1, "frame row %lld hit %d times", (long long)h, hit[(size_t)h]);
        const int64_t c = fr_frame_to_canvas(h, cb, sb);
        CHECK(c >= 0 && c < Hc && fr_canvas_to_frame(c, cb, sb) == h, "round trip of frame row %lld", (long long)h);
      }
      n += Hc;
    }
  return n;
}

static int64_t check_plan() {
  const int dims[] = {21, 22, 137, 981};
  int64_t n = 0;
  for (int dim : dims) {
    const int R = fr_block_rows(dim);
    CHECK(R >= 1 && R <= kFrMaxRows && (int64_t)R * dim <= kFrStageFloats, "dim %d: %d rows per block", dim, R);
    CHECK(R == kFrMaxRows || (int64_t)(R + 1) * dim > kFrStageFloats, "dim %d: the block fills the stage", dim);
    const int64_t rows[] = {1, 2, R - 1, R, R + 1, 3 * (int64_t)R + 5, 4096, 13 * 16 * 9};
    for (int mis = 0; mis < 4; ++mis)
      for (int64_t Hf : rows) {
        if (Hf < 1) continue;
        const uint64_t w0 = 4096 + (uint64_t)mis;  // the frame's base, in words
        std::vector<unsigned char> cover((size_t)(Hf * dim), 0);
        for (int64_t r0 = 0; r0 < Hf; r0 += R) {
          const int nr = (int)(Hf - r0 < R ? Hf - r0 : R), cnt = nr * dim;
          const uint64_t w = w0 + (uint64_t)(r0 * dim);
          const FrSpan sp = fr_span(w, cnt);
          CHECK(sp.head >= 0 && sp.head <= 3 && sp.tail >= 0 && sp.tail <= 3 && sp.nvec >= 0, "span parts");
          CHECK(sp.head + 4 * sp.nvec + sp.tail == cnt, "span length");
          CHECK(sp.nvec == 0 || (w + sp.head) % 4 == 0, "vector loads are 16-byte aligned");
          CHECK((sp.pad + sp.head) % 4 == 0 && sp.pad >= 0 && sp.pad <= 3, "LDS slots are 16-byte aligned");
          CHECK(sp.pad + cnt <= kFrStageWords, "the stage holds the span");
          CHECK(sp.nvec <= kFrStageFloats / 4, "load rounds");
          std::vector<unsigned char> lds((size_t)kFrStageWords, 0);
          auto touch = [&](int e) {  // span element e: loaded once, stored to LDS word pad + e
            CHECK(e >= 0 && e < cnt, "element in the span");
            if (e < 0 || e >= cnt) return;
            cover[(size_t)(r0 * dim + e)]++;
            lds[(size_t)(sp.pad + e)]++;
          };
          for (int t = 0; t < sp.head; ++t) touch(t);
          for (int v = 0; v < sp.nvec; ++v)
            for (int q = 0; q < 4; ++q) touch(sp.head + 4 * v + q);
          for (int t = 0; t < sp.tail; ++t) touch(sp.head + 4 * sp.nvec + t);
          for (int e = 0; e < cnt; ++e) CHECK(lds[(size_t)(sp.pad + e)] == 1, "LDS word of element %d", e);
        }
        for (size_t e = 0; e < cover.size(); ++e)
          CHECK(cover[e] == 1, "dim %d mis %d rows %lld: element %zu covered %d times", dim, mis, (long long)Hf, e,
                cover[e]);
        n += Hf * dim;
      }
  }
  CHECK(fr_block_rows(0) == 0 && fr_block_rows(kFrStageFloats + 1) == 0 && fr_block_rows(kFrStageFloats) == 1,
        "rows that do not fit the stage have no plan");
  // the row of a span element by the multiply-high
  for (int dim : {1, 2, 3, 21, 22, 137, 981, 4096, 8191, 8192}) {
    const uint32_t magic = fr_div_magic(dim);
    for (int e = 0; e < kFrStageWords; ++e)
      CHECK(fr_div(e, dim, magic) == (uint32_t)(e / dim), "fr_div(%d, %d) = %u", e, dim, fr_div(e, dim, magic));
  }
  // a span shorter than its head
  for (int mis = 0; mis < 4; ++mis)
    for (int cnt = 1; cnt < 8; ++cnt) {
      const FrSpan sp = fr_span(64 + mis, cnt);
      CHECK(sp.head + 4 * sp.nvec + sp.tail == cnt && sp.head <= cnt, "short span %d at %d", cnt, mis);
    }
  return n;
}

int main() {
  const int rules = check_rules();
  printf("rules: cases %d\n", rules);
  const int64_t rows = check_mapping();
  printf("mapping: canvas_rows %lld\n", (long long)rows);
  const int64_t elems = check_plan();
  printf("plan: elements %lld\n", (long long)elems);
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("feat_rows ok\n");
  return 0;
}
