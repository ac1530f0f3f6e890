// capi_host.h -- what the host units of the C-ABI share: capi.hip (the context, the
// single-frame path, the readbacks), capi_batch.hip (the lanes, the pipeline, the batch
// entry points) and capi_vosch.hip (normals, RSD, GRSD, VOSCH).  Host only; private to them.
#pragma once
#include <string>

#include "c3h_internal.h"

namespace c3h {

inline int fail(c3h_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}
inline int hip_fail(c3h_ctx* ctx, const char* what, hipError_t e) {
  return fail(ctx, C3H_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(expr)                                          \
  do {                                                        \
    hipError_t e_ = (expr);                                   \
    if (e_ != hipSuccess) return c3h::hip_fail(ctx, #expr, e_); \
  } while (0)

template <class T>
int ensure(c3h_ctx* ctx, DevBuf<T>& b, size_t n) {
  bool in_free = false;
  const hipError_t e = b.reserve(n, &in_free);
  if (e == hipSuccess) return C3H_OK;
  if (in_free) return hip_fail(ctx, "hipFree", e);
  return fail(ctx, C3H_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
}

// the pipeline of c3h_run_frames / c3h_stream_frames (capi_batch.hip)
int pipe_quiesce(c3h_ctx* ctx);
int pipe_flush(c3h_ctx* ctx);

// entry points that touch a context's buffers first drain its open frame stream
#define QUIESCE(ctx)                            \
  do {                                          \
    int rq_ = c3h::pipe_quiesce(ctx);           \
    if (rq_ != C3H_OK) return rq_;              \
  } while (0)

#define ENSURE(buf, n)                            \
  do {                                            \
    int rc_ = c3h::ensure(ctx, buf, (size_t)(n)); \
    if (rc_ != C3H_OK) return rc_;                \
  } while (0)

// ---- timing ------------------------------------------------------------------------
struct Timed {
  c3h_ctx* ctx;
  c3h::Timer* T;
  int slot, weight;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  hipStream_t st;
  Timed(c3h_ctx* c, int s, int w = 1, hipStream_t on = nullptr)
      : ctx(c), T(c->parent ? &c->parent->timer : &c->timer), slot(s), weight(w), st(on ? on : c->stream) {
    if (!(T->mask >> (s + 1) & 1) || c->capture) return;
    std::lock_guard<std::mutex> g(T->mu);
    if (T->pool.empty()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess) return;
      if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        return;
      }
      T->pool.push_back({a, b});
    }
    ev = T->pool.back();
    T->pool.pop_back();
    (void)hipEventRecord(ev.first, st);  // on the stream the kernels run on
  }
  ~Timed() {
    if (!ev.first) return;
    (void)hipEventRecord(ev.second, st);
    std::lock_guard<std::mutex> g(T->mu);
    T->pending[slot].push_back(c3h::TimedPair{ev.first, ev.second, weight});
  }
};

// a sensor_msgs/PointCloud2 message's geometry and field offsets (every PointCloud2 entry point)
inline int pc2_check(c3h_ctx* ctx, uint32_t height, uint32_t width, uint32_t point_step, uint32_t row_step,
                     const int32_t off[4]) {
  if (!off) return fail(ctx, C3H_ERR_ARG, "pointcloud2: no field offsets");
  for (int k = 0; k < 4; ++k)
    if ((k < 3 && off[k] < 0) || off[k] + 4 > (int64_t)point_step)
      return fail(ctx, C3H_ERR_ARG, "pointcloud2: field x/y/z missing or outside point_step");
  if (height > 1 && (uint64_t)row_step < (uint64_t)width * point_step)
    return fail(ctx, C3H_ERR_ARG, "pointcloud2: row_step < width * point_step");
  return C3H_OK;
}

// the single-frame path's steps the batch code and the GRSD front sequence (capi.hip)
int mode_schedule(int r1, int r2, int r3, int rotate, int* modes);
bool extract_params_ok(const c3h_extract_params* p);
int extract_frames(c3h_ctx* ctx, const uint32_t* const* grids, int nf, const c3h_extract_params* p,
                   int32_t subdiv_out[3], int64_t* hist_num);
int search_frames(c3h_ctx* ctx, int nf, const int32_t range[3], int32_t thr, int32_t rotate,
                  c3h_det* const* d_outs, int clean);
int grsd_frame_head(c3h_ctx* ctx, const c3h_grsd_params* p, int32_t sb[3], int64_t* Hout, float* inv_s);
int search_setup_dev(c3h_ctx* ctx, const float* axis_p, const float* var, int32_t D, int32_t F,
                     const float* axis_q, int32_t M, int32_t r, const float* fmax, int32_t fmax_len, int32_t D_user);

}  // namespace c3h
