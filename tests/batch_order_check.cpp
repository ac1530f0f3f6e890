// batch_order_check.cpp -- csrc/batch_order.h on the host (its own main; built with
// -fsanitize=address,undefined by test_batch_order_cpu.py and run as a program).
//
// For B in {1, 2, 3, 32}, nframes 1 .. 4 B + 1, draining and not:
//  - every frame index appears exactly once over all chunks;
//  - chunks other than a draining call's last are in natural order;
//  - a draining call's last chunk has the last frame in slot 0, the rest in order behind it;
//  - from the start sequence number, the last chunk's buffer set (seq + nchunks - 1) % 4 is 0;
//  - the header agrees, slot by slot, with a literal transcription of the expressions the batch
//    drivers carried before they shared it (ref_chunk_frames, ref_pipe_seq).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "batch_order.h"

namespace {

long long g_checks = 0;

#define CHECK(cond)                                                                         \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(cond)) {                                                                          \
      std::fprintf(stderr, "%s:%d: %s (B %d nframes %d drain %d ch %d)\n", __FILE__, __LINE__, #cond, B, nframes, \
                   (int)drain, ch);                                                         \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

// the former chunk_frames of the grid-frames driver, on frame indices (nchunks < 0: natural
// order throughout); returns the chunk's frame count
int ref_chunk_frames(int nframes, int B, int nchunks, int ch, int* frames) {
  const int f0 = ch * B, nb = std::min(B, nframes - f0);
  for (int j = 0; j < nb; ++j) {
    const int fi = (ch == nchunks - 1) ? (j == 0 ? f0 + nb - 1 : f0 + j - 1) : f0 + j;
    frames[j] = fi;
  }
  return nb;
}

// the former start of a draining call on an empty pipeline
uint64_t ref_pipe_seq(int nchunks) {
  constexpr int kPipeDepth = 4;
  return (uint64_t)((kPipeDepth - (nchunks - 1) % kPipeDepth) % kPipeDepth);
}

}  // namespace

int main() {
  static_assert(c3h::kPipeDepth == 4, "four buffer sets");
  const int Bs[] = {1, 2, 3, 32};
  for (int B : Bs)
    for (int nframes = 1; nframes <= 4 * B + 1; ++nframes)
      for (int d = 0; d < 2; ++d) {
        const bool drain = d != 0;
        int ch = -1;
        const int nchunks = c3h::chunk_count(nframes, B);
        CHECK(nchunks == (nframes + B - 1) / B);
        std::vector<int> seen((size_t)nframes, 0);
        for (ch = 0; ch < nchunks; ++ch) {
          const int f0 = ch * B;
          const int nb = c3h::chunk_size(nframes, B, ch);
          std::vector<int> ref((size_t)B, -1);  // exactly B slots: a longer chunk overruns under ASan
          CHECK(ref_chunk_frames(nframes, B, drain ? nchunks : -1, ch, ref.data()) == nb);
          CHECK(nb >= 1 && nb <= B && f0 + nb <= nframes);
          for (int j = 0; j < nb; ++j) {
            const int fi = c3h::chunk_frame(nframes, B, ch, j, drain);
            CHECK(fi == ref[(size_t)j]);
            CHECK(fi >= 0 && fi < nframes);
            seen[(size_t)fi]++;
            if (drain && ch == nchunks - 1)
              CHECK(fi == (j == 0 ? nframes - 1 : f0 + j - 1));
            else
              CHECK(fi == f0 + j);
          }
        }
        ch = -1;
        for (int f = 0; f < nframes; ++f) CHECK(seen[(size_t)f] == 1);
        const uint64_t seq = c3h::drain_start_seq(nchunks);
        CHECK(seq == ref_pipe_seq(nchunks));
        CHECK(seq < 4 && (seq + (uint64_t)nchunks - 1) % 4 == 0);
      }
  std::printf("checks: %lld\nbatch_order ok\n", g_checks);
  return 0;
}
