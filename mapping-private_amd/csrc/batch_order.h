// batch_order.h -- which frame goes into which slot of which batch, and on which buffer set
// a call's batches start.  Host only, plain C++ (tests/batch_order_check.cpp compiles it alone).
#pragma once
#include <algorithm>
#include <cstdint>

namespace c3h {

// buffer sets of the software pipeline: batch number s is prepared on set s % kPipeDepth
constexpr int kPipeDepth = 4;

inline int chunk_count(int nframes, int B) { return (nframes + B - 1) / B; }
inline int chunk_size(int nframes, int B, int ch) { return std::min(B, nframes - ch * B); }

// The frame in slot j of chunk ch (B frames per chunk).  Natural order, except in the last
// chunk of a call that completes its frames (last_first): that chunk puts its last frame in
// slot 0 and the rest in order behind it, so the context that runs it ends up holding the last
// frame's state.
inline int chunk_frame(int nframes, int B, int ch, int j, bool last_first) {
  const int f0 = ch * B;
  if (!last_first || ch != chunk_count(nframes, B) - 1) return f0 + j;
  return j == 0 ? f0 + chunk_size(nframes, B, ch) - 1 : f0 + j - 1;
}

// The batch number a draining call of nchunks batches starts from on an empty pipeline: its
// last batch then lands on set 0, the calling context.
inline uint64_t drain_start_seq(int nchunks) {
  return (uint64_t)((kPipeDepth - (nchunks - 1) % kPipeDepth) % kPipeDepth);
}

}  // namespace c3h
