// feat_front.hip -- the front of a batch of caller-computed feature rows
// (c3h_run_feature_frames / c3h_stream_feature_frames: SearchObj::setData, search.cpp:539-658,
// as setVOSCH / setConVOSCH / setGRSD call it, search_new.h:34-126, over a whole batch).
//
// One launch per batch, ahead of the batch's first tick.  It puts the frames' rows into a
// buffer set in the form the tick's gate and compress roles expect of an extract:
//
//   exist  [frame][canvas row]  exist_voxel_num (the caller's, or by rule); 0 outside the frame
//   has    [frame][canvas row]  1 when the row holds an element != 0 (-0 counts as 0), else 0
//   rows   [frame][..]          the canvas rows with data (any order), cnt[frame] of them
//   out    [frame][canvas row][dim]  the rows with data, at their canvas index
//   lim    [frame][4]           the frame's own subdivision counts (the gate's position limits)
//
// exist 0 does not mean "no data" for such rows (a GRSD row of few transitions has exist 0 and
// non-zero features, and searchPart adds it), so the score role skips rows by `has` while the
// gate sums `exist`.  A row without data compresses to +0 in every column and the box sums
// start at +0, so skipping it gives the bits adding it would; nothing is zero-filled.
//
// Workgroup (b, f): rows [b * R, (b + 1) * R) of frame f (R = fr_block_rows(dim)) as one flat
// span of floats, streamed once through LDS: the head is peeled to 16-byte alignment (rows of
// 137 floats are not aligned), the body goes in non-temporal 16-byte loads that are all issued
// before the first is consumed, the tail in single words (feat_rows.h).  The workgroups of a
// frame also write the zeros of the canvas rows outside it: the buffer sets rotate, a word
// left by the previous occupant would be a wrong result.
#include <algorithm>
#include <climits>

#include "c3h_internal.h"
#include "feat_rows.h"

namespace c3h {
namespace {

typedef float fr_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kFrVecs = kFrStageFloats / 4 / kBlock;  // 16-byte loads per thread of a full stage
static_assert(kFrVecs * 4 * kBlock == kFrStageFloats, "the stage is a whole number of load rounds");
static_assert(kFrMaxRows <= kBlock, "a thread per row of a block");

__global__ __launch_bounds__(kBlock) void feat_front_kernel(FeatFront a) {
  __shared__ __attribute__((aligned(16))) float stage[kFrStageWords];
  __shared__ int has_s[kFrMaxRows];   // the row holds an element != 0
  __shared__ int crow_s[kFrMaxRows];  // its canvas row
  __shared__ int wcnt_s[kBlock / 64 + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f = blockIdx.y;
  const int dim = a.dim;
  const int cb[3] = {a.cb[0], a.cb[1], a.cb[2]};
  const int sb[3] = {a.sb[f][0], a.sb[f][1], a.sb[f][2]};
  const int64_t Hc = (int64_t)cb[0] * cb[1] * cb[2], Hf = (int64_t)sb[0] * sb[1] * sb[2];
  int32_t* __restrict__ exist = a.exist + f * a.s_h;
  int32_t* __restrict__ has = a.has + f * a.s_h;
  if (blockIdx.x == 0 && tid < 4) a.lim[4 * f + tid] = tid < 3 ? sb[tid] : 0;
  // canvas rows outside the frame: 0 in both arrays (a frame that fills the canvas has none)
  if (Hf != Hc)
    for (int64_t c = (int64_t)blockIdx.x * kBlock + tid; c < Hc; c += (int64_t)gridDim.x * kBlock)
      if (fr_canvas_to_frame(c, cb, sb) < 0) {
        exist[c] = 0;
        has[c] = 0;
      }
  const int R = a.R;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  if (r0 >= Hf) return;
  const int nr = (int)(Hf - r0 < R ? Hf - r0 : R);
  const int n = nr * dim;  // <= kFrStageFloats
  const float* __restrict__ src = a.feat[f] + r0 * dim;
  has_s[tid] = 0;  // (ahead of the barrier behind the stage's fill)
  const FrSpan sp = fr_span((uint64_t)(uintptr_t)src >> 2, n);
  float* st = stage + sp.pad;  // span element e at st[e]
  {
    const fr_f32x4* v4 = reinterpret_cast<const fr_f32x4*>(src + sp.head);
    fr_f32x4 reg[kFrVecs];
#pragma unroll
    for (int k = 0; k < kFrVecs; ++k) {
      const int v = tid + k * kBlock;
      reg[k] = v < sp.nvec ? __builtin_nontemporal_load(v4 + v) : fr_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float edge = 0.0f;  // the head's and the tail's words: threads 0 .. 2 and 4 .. 6
    const int te = tid - 4;
    if (tid < sp.head) edge = __builtin_nontemporal_load(src + tid);
    else if (te >= 0 && te < sp.tail) edge = __builtin_nontemporal_load(src + sp.head + 4 * sp.nvec + te);
#pragma unroll
    for (int k = 0; k < kFrVecs; ++k) {
      const int v = tid + k * kBlock;
      if (v < sp.nvec) *reinterpret_cast<fr_f32x4*>(st + sp.head + 4 * v) = reg[k];
    }
    if (tid < sp.head) st[tid] = edge;
    else if (te >= 0 && te < sp.tail) st[sp.head + 4 * sp.nvec + te] = edge;
  }
  __syncthreads();
  // has-data flags: one flat pass over the span (consecutive lanes, consecutive words); the
  // element's row by a multiply-high, the division by dim being the pass's whole cost otherwise
  const uint32_t magic = a.magic;
  for (int e = tid; e < n; e += kBlock)
    if (st[e] != 0.0f) has_s[fr_div(e, dim, magic)] = 1;
  __syncthreads();
  // a thread per row: exist, the flag, the row's place in the list
  bool data = false;
  int64_t c = 0;
  if (tid < nr) {
    c = fr_frame_to_canvas(r0 + tid, cb, sb);
    data = has_s[tid] != 0;
    exist[c] = a.exist_in[f] ? a.exist_in[f][r0 + tid] : fr_exist_rule(st + tid * dim, a.rule);
    has[c] = data ? 1 : 0;
    crow_s[tid] = (int)c;
  }
  const unsigned long long m = __ballot(data);
  if (lane == 0) wcnt_s[wave] = __popcll(m);
  __syncthreads();
  if (tid == 0) {  // one returning atomic per workgroup
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) tot += wcnt_s[w];
    wcnt_s[kBlock / 64] = tot ? (int)atomicAdd(&a.cnt[f], (uint32_t)tot) : 0;
    wcnt_s[kBlock / 64 + 1] = tot;
  }
  __syncthreads();
  if (wcnt_s[kBlock / 64 + 1] == 0) return;  // a block without data (most of a surface scene's)
  if (data) {
    int base = wcnt_s[kBlock / 64];
    for (int w = 0; w < wave; ++w) base += wcnt_s[w];
    a.rows[f * a.s_h + base + __popcll(m & ((1ull << lane) - 1))] = (int32_t)c;
  }
  // the rows with data, from the stage to their canvas index
  float* __restrict__ out = a.out + f * a.s_out;
  for (int e = tid; e < n; e += kBlock) {
    const int r = (int)fr_div(e, dim, magic);
    if (has_s[r]) out[(int64_t)crow_s[r] * dim + (e - r * dim)] = st[e];
  }
}

}  // namespace

bool feat_front_ok(int dim) { return fr_block_rows(dim) > 0; }

hipError_t launch_feat_front(const FeatFront& a, hipStream_t s) {
  if (a.nf < 1) return hipSuccess;
  const int R = fr_block_rows(a.dim);
  if (R < 1 || a.R != R || a.magic != fr_div_magic(a.dim) || a.nf > kMaxBatch) return hipErrorInvalidValue;
  int64_t hmax = 0;
  const int64_t Hc = (int64_t)a.cb[0] * a.cb[1] * a.cb[2];
  for (int f = 0; f < a.nf; ++f) {
    for (int k = 0; k < 3; ++k)
      if (a.sb[f][k] < 0 || a.sb[f][k] > a.cb[k]) return hipErrorInvalidValue;  // rows past the canvas
    hmax = std::max(hmax, (int64_t)a.sb[f][0] * a.sb[f][1] * a.sb[f][2]);
  }
  if (Hc < 1 || Hc > INT32_MAX || a.s_h < Hc || a.s_out < Hc * a.dim) return hipErrorInvalidValue;
  // a workgroup per row block of the largest frame; at least enough to zero a canvas quickly
  const int64_t gx = std::max<int64_t>((hmax + R - 1) / R, std::min<int64_t>((Hc + kBlock - 1) / kBlock, 64));
  feat_front_kernel<<<dim3((unsigned)gx, (unsigned)a.nf), kBlock, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace c3h
