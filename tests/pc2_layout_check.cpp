// pc2_layout_check.cpp -- csrc/pc2_layout.h on the host (its own main; built with
// -fsanitize=address,undefined by test_pointcloud2_frames_cpu.py): the plan's classification,
// the point index -> byte offset mapping against 64-bit division, the three load forms on the
// same random bytes, and the highest byte any form touches.  Every message is allocated at its
// exact size, so a load past it is an AddressSanitizer error as well as a failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pc2_layout.h"

using namespace c3h;

static long g_checks = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    ++g_checks;                                                                \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

// the accessor the kernels' loads go through, on host bytes: every load is bounds-checked
// against the message and the highest byte touched is kept
struct HostMem {
  const uint8_t* p;
  uint64_t size;
  mutable uint64_t hi = 0;
  mutable bool any = false;
  void touch(uint64_t o, uint64_t n) const {
    CHECK(o + n <= size);
    if (!any || o + n - 1 > hi) hi = o + n - 1;
    any = true;
  }
  void ld16(uint64_t o, uint32_t* out) const {
    touch(o, 16);
    std::memcpy(out, p + o, 16);
  }
  uint32_t ld4(uint64_t o) const {
    touch(o, 4);
    uint32_t v;
    std::memcpy(&v, p + o, 4);
    return v;
  }
  uint32_t ld1(uint64_t o) const {
    touch(o, 1);
    return p[o];
  }
};

template <int kForm, int kNP>
static void words(const HostMem& m, uint64_t o, const Pc2Plan& L, uint32_t out[4]) {
  const Pc2Raw<kForm, kNP> r = pc2_load<kForm, kNP>(m, o, L);
  pc2_extract<kForm, kNP>(r, L, out);
}
static void words_by_plan(const HostMem& m, uint64_t o, const Pc2Plan& L, uint32_t out[4]) {
  if (L.form == kPc2Vec16) {
    if (L.npiece == 2) words<kPc2Vec16, 2>(m, o, L, out);
    else words<kPc2Vec16, 1>(m, o, L, out);
  } else if (L.form == kPc2Dword) {
    words<kPc2Dword, 1>(m, o, L, out);
  } else {
    words<kPc2Bytes, 1>(m, o, L, out);
  }
}
// the reference: pc2_convert_kernel's byte assembly written out
static void words_ref(const uint8_t* rec, const int32_t off[4], int big, uint32_t out[4]) {
  for (int k = 0; k < 4; ++k) {
    if (off[k] < 0) {
      out[k] = 0;
      continue;
    }
    const uint8_t* b = rec + off[k];
    out[k] = big ? ((uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3])
                 : ((uint32_t)b[3] << 24 | (uint32_t)b[2] << 16 | (uint32_t)b[1] << 8 | b[0]);
  }
}

struct Lay {
  uint32_t step;
  int32_t off[4];
};
static const Lay kKinect{32, {0, 4, 8, 16}}, kFloat4{16, {0, 4, 8, 12}}, kDword{20, {4, 8, 12, 16}},
    kOdd{19, {1, 5, 9, 14}}, kKinectNoRgb{32, {0, 4, 8, -1}}, kThree{48, {0, 16, 32, 36}};

int main() {
  // ---- plan classification ---------------------------------------------------------------
  long n_plan = g_checks;
  {
    Pc2Plan p = pc2_plan(kKinect.step, kKinect.off, 0, 0x7f0000001000ull, 640 * 32 + 16);
    CHECK(p.form == kPc2Vec16 && p.npiece == 2 && p.piece[0] == 0 && p.piece[1] == 16);
    CHECK(p.sel[0] == 0 && p.sel[1] == 1 && p.sel[2] == 2 && p.sel[3] == 4);
    p = pc2_plan(kFloat4.step, kFloat4.off, 0, 0x1000, 0);
    CHECK(p.form == kPc2Vec16 && p.npiece == 1 && p.sel[3] == 3);
    p = pc2_plan(kKinectNoRgb.step, kKinectNoRgb.off, 0, 0x1000, 0);
    CHECK(p.form == kPc2Vec16 && p.npiece == 1 && p.sel[3] == -1);
    p = pc2_plan(kDword.step, kDword.off, 0, 0x1000, 160 * 20 + 4);
    CHECK(p.form == kPc2Dword);
    p = pc2_plan(kOdd.step, kOdd.off, 0, 0x1000, 0);
    CHECK(p.form == kPc2Bytes);
    for (const Lay* l : {&kKinect, &kFloat4, &kDword, &kOdd})  // any big-endian layout
      CHECK(pc2_plan(l->step, l->off, 1, 0x1000, 0).form == kPc2Bytes);
    // a misaligned base pointer demotes VEC16 (to DWORD at 4, to BYTES at 1 or 2), so does a row step
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1008, 0).form == kPc2Dword);
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1004, 0).form == kPc2Dword);
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1002, 0).form == kPc2Bytes);
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1001, 0).form == kPc2Bytes);
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1000, 640 * 32 + 4).form == kPc2Dword);
    CHECK(pc2_plan(kKinect.step, kKinect.off, 0, 0x1000, 640 * 32 + 2).form == kPc2Bytes);
    CHECK(pc2_plan(kDword.step, kDword.off, 0, 0x1002, 0).form == kPc2Bytes);
    // wanted fields in three pieces: one load per field is less
    CHECK(pc2_plan(kThree.step, kThree.off, 0, 0x1000, 0).form == kPc2Dword);
  }
  n_plan = g_checks - n_plan;

  // ---- index -> byte offset ----------------------------------------------------------------
  long n_map = g_checks;
  {
    const uint32_t widths[] = {1, 7, 160, 640}, pads[] = {0, 4, 16, 20}, steps[] = {16, 19, 20, 32};
    for (uint32_t w : widths)
      for (uint32_t pad : pads)
        for (uint32_t ps : steps) {
          const uint32_t h = w == 1 ? 1000 : (w == 7 ? 333 : 120), rs = w * ps + pad;
          const Pc2Frame f = pc2_frame(h, w, ps, rs);
          CHECK((f.magic == 0) == (pad == 0));
          for (uint32_t i = 0; i < h * w; ++i) {
            const uint64_t row = (uint64_t)i / w, col = (uint64_t)i % w;
            CHECK(pc2_offset(i, f, ps) == row * rs + col * ps);
          }
        }
    // every index below 2^24 at widths whose reciprocal is the least exact: around powers of
    // two, odd, and the largest a padded message can have (height 2)
    const uint32_t hard[] = {3, 641, 4097, 65535, (1u << 23) - 1, 5592405u};
    for (uint32_t w : hard) {
      const Pc2Frame f = pc2_frame(2, w, 32, w * 32 + 16);
      CHECK(f.magic != 0);
      uint32_t row = 0, col = 0;
      for (uint32_t i = 0; i < (1u << 24); ++i) {  // (row, col) carried along: no division here either
        if (pc2_row(i, f.magic, f.shift) != row) {
          std::fprintf(stderr, "row of %u at width %u\n", i, w);
          return 1;
        }
        if (++col == w) col = 0, ++row;
      }
      ++g_checks;
    }
    // height 1 at widths near 2^24: flat whatever row_step says, offsets beyond 32 bits
    for (uint32_t w : {(1u << 24) - 1, (1u << 24) - 2, (1u << 24) - 640}) {
      const Pc2Frame f = pc2_frame(1, w, 304, 12345);
      CHECK(f.magic == 0);
      for (uint32_t i : {0u, 1u, w / 2, w - 2, w - 1}) CHECK(pc2_offset(i, f, 304) == (uint64_t)i * 304);
      CHECK(pc2_msg_bytes(1, w, 304, 12345) == (uint64_t)w * 304);
    }
    CHECK(pc2_msg_bytes(0, 640, 32, 640 * 32) == 0 && pc2_msg_bytes(3, 0, 32, 0) == 0);
    CHECK(pc2_msg_bytes(120, 160, 32, 160 * 32 + 16) == 119ull * (160 * 32 + 16) + 160 * 32);
  }
  n_map = g_checks - n_map;

  // ---- field extraction and bounds ---------------------------------------------------------
  long n_words = g_checks;
  {
    std::mt19937 rng(1234);
    const Lay* lays[] = {&kKinect, &kFloat4, &kDword, &kOdd, &kKinectNoRgb, &kThree};
    for (const Lay* l : lays)
      for (int big = 0; big < 2; ++big)
        for (uint32_t pad : {0u, 4u, 16u, 20u}) {
          const uint32_t h = 5, w = 37, rs = w * l->step + pad;
          const uint64_t size = pc2_msg_bytes(h, w, l->step, rs);  // the last row is short
          std::vector<uint8_t> heap(size);
          for (auto& b : heap) b = (uint8_t)rng();
          const Pc2Frame f = pc2_frame(h, w, l->step, rs);
          // the plan the library would make for a 16-byte aligned message, and the two lower
          // forms forced: all give the reference's words, none reads past the message
          const Pc2Plan best = pc2_plan(l->step, l->off, big, 0, f.magic ? rs : 0);
          Pc2Plan forms[3] = {best, best, best};
          int nforms = 1;
          if (best.form == kPc2Vec16) forms[nforms++].form = kPc2Dword;
          if (best.form != kPc2Bytes) forms[nforms++].form = kPc2Bytes;
          for (int q = 0; q < nforms; ++q) {
            HostMem m{heap.data(), size};
            for (uint32_t i = 0; i < h * w; ++i) {
              const uint64_t o = pc2_offset(i, f, l->step);
              uint32_t got[4], ref[4];
              words_by_plan(m, o, forms[q], got);
              words_ref(heap.data() + (uint64_t)(i / w) * rs + (uint64_t)(i % w) * l->step, l->off, big, ref);
              CHECK(std::memcmp(got, ref, 16) == 0);
            }
            CHECK(m.any && m.hi < size);
            // VEC16 reads whole pieces: the last record's last piece ends with the message
            if (forms[q].form == kPc2Vec16 && (l->step & 15) == 0 && forms[q].piece[forms[q].npiece - 1] + 16 == (int)l->step)
              CHECK(m.hi == size - 1);
          }
        }
  }
  n_words = g_checks - n_words;

  std::printf("plan: %ld\nmapping: %ld\nwords: %ld\npc2_layout ok\n", n_plan, n_map, n_words);
  return 0;
}
