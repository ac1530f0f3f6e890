// capi_batch.hip -- the batch half of the C-ABI (capi.hip holds the context, the single-frame
// path and the readbacks): the frame lanes, the software pipeline of tick launches, and the
// three families of batch entry points -- grids in (c3h_run_frames, c3h_stream_frames), feature
// rows in (c3h_run_feature_frames) and points in (c3h_run_point_frames,
// c3h_run_pointcloud2_frames).  Host code only: every kernel lives in another unit.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <thread>

#include "batch_order.h"
#include "capi_host.h"
#include "feat_rows.h"

using namespace c3h;

namespace {

// child contexts lanes[0 .. n-1] exist and carry the context's search setup and rank
int ensure_lanes(c3h_ctx* ctx, int n) {
  while ((int)ctx->lanes.size() < n) {
    c3h_ctx* c = nullptr;
    int rc = c3h_create(ctx->device, &c);
    if (rc != C3H_OK) return fail(ctx, rc, "c3h_run_frames: lane context");
    c->parent = ctx;
    ctx->lanes.push_back(c);
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->lane_ev.push_back(e);
  }
  bool synced = false;
  for (int l = 0; l < n; ++l) {
    c3h_ctx* c = ctx->lanes[l];
    if (c->setup_version != ctx->setup_version || !c->have_setup) {
      if (!synced) {  // pipelined batches of this lane may still be queued on the parent's stream
        HIPCHK(hipStreamSynchronize(ctx->stream));
        synced = true;
      }
      int rc = search_setup_dev(c, ctx->h_axis_p.empty() ? nullptr : ctx->h_axis_p.data(),
                                ctx->h_var.empty() ? nullptr : ctx->h_var.data(), ctx->D, ctx->F,
                                ctx->h_axis_q.data(), ctx->M, ctx->r,
                                ctx->h_fmax.empty() ? nullptr : ctx->h_fmax.data(), (int)ctx->h_fmax.size(),
                                ctx->D_user);
      if (rc != C3H_OK) return fail(ctx, rc, std::string("c3h_run_frames: lane setup: ") + c->err);
      c->setup_version = ctx->setup_version;
    }
    if (c->rank != ctx->rank) {
      int rc = c3h_set_rank(c, ctx->rank);
      if (rc != C3H_OK) return rc;
    }
  }
  return C3H_OK;
}

// c3h_set_remove_overlap: the launch that passes the records of nb searched frames (outs)
// through removeOverlap; it goes behind those searches on their stream
c3h::RemoveOverlapFrames overlap_args(const c3h_ctx* ctx, const int32_t range[3], c3h_det* const* outs, int nb) {
  c3h::RemoveOverlapFrames ro{};
  ro.M = std::max(ctx->M, 1);
  ro.nf = nb;
  ro.rank = ctx->rank;
  ro.r1 = range[0];
  ro.r2 = range[1];
  ro.r3 = range[2];
  for (int f = 0; f < nb; ++f) ro.outs[f] = outs[f];
  return ro;
}

bool overlap_wanted(const c3h_ctx* ctx) { return ctx->remove_overlap && ctx->rank >= 2; }

// The records of nb frames whose search on context c returned rc: removeOverlap behind that
// search where ctx (the caller's context) wants it.  Returns rc, or the launch's error (in c).
int overlap_behind(const c3h_ctx* ctx, c3h_ctx* c, const int32_t range[3], c3h_det* const* outs, int nb, int rc) {
  if (rc < 0 || !overlap_wanted(ctx)) return rc;
  const hipError_t e = c3h::launch_remove_overlap_frames(overlap_args(ctx, range, outs, nb), c->stream);
  return e == hipSuccess ? rc : hip_fail(c, "launch_remove_overlap_frames", e);
}

// the batch entry points' limit: the per-slot form holds a list on the lanes of one wave
int overlap_rank_check(c3h_ctx* ctx, const char* who) {
  if (ctx->remove_overlap && ctx->rank > 64)
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": c3h_set_remove_overlap needs rank <= 64");
  return C3H_OK;
}

// Software-pipelined batches (pipeline.hip).  Batch number s is prepared on buffer set
// s % 4 (set 0 = this context; kPipeDepth, batch_order.h) and runs as the occupancy role of
// one tick, the tile role of the next, compress+gate of the one after and scoring + rank-1
// argmax of the fourth.
// All buffer sets work on this context's stream, so ticks order themselves; the host
// only enqueues.  The pipeline persists across c3h_stream_frames calls (a continuous
// frame source keeps it full); c3h_run_frames and c3h_stream_flush drain it.
c3h_ctx* pipe_set(c3h_ctx* ctx, uint64_t seq) {
  const int set = (int)(seq % kPipeDepth);
  return set == 0 ? ctx : ctx->lanes[set - 1];
}

// lane contexts enqueue on the parent's stream while a pipeline call runs
struct PipeScope {
  c3h_ctx* ctx;
  hipStream_t saved[kPipeDepth - 1];
  explicit PipeScope(c3h_ctx* c) : ctx(c) {
    ctx->pipe_busy = true;
    for (int l = 0; l < kPipeDepth - 1 && l < (int)ctx->lanes.size(); ++l) {
      saved[l] = ctx->lanes[l]->stream;
      ctx->lanes[l]->stream = ctx->stream;
    }
  }
  ~PipeScope() {
    for (int l = 0; l < kPipeDepth - 1 && l < (int)ctx->lanes.size(); ++l) ctx->lanes[l]->stream = saved[l];
    ctx->pipe_busy = false;
  }
};

// one tick: the occupancy role of `fresh` (nullable) and the next role of every batch in
// flight; afterwards every batch is one stage older and finished batches leave
int pipe_tick(c3h_ctx* ctx, const c3h_ctx::PipeBatch* fresh) {
  c3h::TickParts tp;
  tp.prof = &ctx->prof;
  // a feature-row batch has no occupancy and no tile role (its front kernel wrote what they
  // produce): it joins at the compress + gate slot of this very tick
  const bool rows_in = fresh && fresh->rows_in;
  if (rows_in) {
    ctx->pipe.push_back(*fresh);
    ctx->pipe.back().age = 2;
  }
  if (fresh && !fresh->stamped && !rows_in) tp.occ = &fresh->l;
  for (auto& b : ctx->pipe) {
    if (b.age == 1) {
      tp.tile = &b.l;
      tp.tile_mapped = b.mapped;
    }
    if (b.age == 2) {
      tp.gate = &b.q;
      tp.comp = &b.sc;
    }
    if (b.age == 3) tp.score = b.rows_in ? &b.qs : &b.q;
  }
  {
    Timed tm(ctx, 5, fresh ? fresh->nf : 0);
    hipError_t e = c3h::launch_tick(tp, ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "launch_tick", e);
  }
  for (auto& b : ctx->pipe) {
    if (b.age == 3 && b.replay) {  // its score role ran in this tick: the lists of its frames
      Timed tm(ctx, 4, b.nf);
      hipError_t e = c3h::launch_replay_frames(b.rp, ctx->stream);
      if (e != hipSuccess) return hip_fail(ctx, "launch_replay_frames", e);
    }
    if (b.age == 3 && b.overlap) {  // removeOverlap on its frames' records, behind the replay
      hipError_t e = c3h::launch_remove_overlap_frames(b.ro, ctx->stream);
      if (e != hipSuccess) return hip_fail(ctx, "launch_remove_overlap_frames", e);
    }
    if (b.age == 2 && b.set) {  // this tick enqueued its gate: slot 0 always, the rest when it keeps them
      b.set->scores_layout = b.layout;
      if (b.q.scores_slot0_only) b.set->scores_layout_rest.clear();
      else b.set->scores_layout_rest = b.layout;
    }
    if (b.age == 1 && b.fix) {  // its tile role ran in this tick: the off-cell fixup before its compress
      hipError_t e = c3h::launch_point_fixup(b.fx, ctx->stream);
      if (e != hipSuccess) return hip_fail(ctx, "launch_point_fixup", e);
    }
  }
  std::vector<c3h_ctx::PipeBatch> next;
  for (auto& b : ctx->pipe)
    if (b.age < (b.nosearch ? 1 : 3)) {
      next.push_back(b);
      next.back().age++;
    }
  if (fresh && !rows_in) {
    next.push_back(*fresh);
    next.back().age = 1;
    next.back().mapped = tp.occ != nullptr;
  }
  ctx->pipe.swap(next);
  return C3H_OK;
}

// the remaining ticks of the batches in flight (inside a PipeScope); an error empties the pipeline
int pipe_drain(c3h_ctx* ctx) {
  while (!ctx->pipe.empty()) {
    int rc = pipe_tick(ctx, nullptr);
    if (rc != C3H_OK) {
      ctx->pipe.clear();
      return rc;
    }
  }
  return C3H_OK;
}

}  // namespace

int c3h::pipe_flush(c3h_ctx* ctx) {
  if (ctx->pipe.empty()) return C3H_OK;
  PipeScope scope(ctx);
  return pipe_drain(ctx);
}

// public entry points that touch this context's buffers drain an open stream first
int c3h::pipe_quiesce(c3h_ctx* ctx) {
  if (ctx->pipe_busy || ctx->pipe.empty()) return C3H_OK;
  return pipe_flush(ctx);
}

namespace {

// The common end of a capture on buffer set c (pipe_prepare, feature_prepare).  False when
// the tick cannot rank the captured search: rank 1 is the score role's fused argmax; at ranks
// 2 .. 64 the score role writes the scores only and the batched replay follows it.  Otherwise
// fresh, whose roles the caller has filled, gets the set, its score layout, and the replay and
// removeOverlap launches that follow its score role.
bool pipe_capture_end(const c3h_ctx* ctx, c3h_ctx* c, const int32_t range[3], c3h_det* const* outs, int nb,
                      c3h_ctx::PipeBatch* fresh) {
  if (!c->cap_argmax && !(c->cap_replay && c->rank >= 2 && !c->cap_q.lists && !c->cap_q.partials)) return false;
  fresh->set = c;
  fresh->layout = c->cap_layout;
  // rank 1: the detections come from the partials, and c3h_get_scores sees slot 0 only
  fresh->q.scores_slot0_only = c->cap_argmax ? 1 : 0;
  fresh->replay = !c->cap_argmax;
  fresh->rp = c->cap_rp;
  fresh->overlap = overlap_wanted(ctx);
  if (fresh->overlap) fresh->ro = overlap_args(ctx, range, outs, nb);
  return true;
}

// Captures nb frames as the next batch on its buffer set (no launch: its tile stamps may
// come from elsewhere first).  Returns > 0 (modes searched), 0 when the configuration does
// not fit the tick (only possible for the first batch of a stream: the caller then runs
// the lanes), < 0 on error.
int pipe_prepare(c3h_ctx* ctx, const uint32_t* const* grids, c3h_det* const* outs, int nb,
                 const c3h_ctx::PipeKey& k, const int32_t* lim, c3h_ctx::PipeBatch* fresh) {
  c3h_ctx* c = pipe_set(ctx, ctx->pipe_seq);
  c->capture = true;
  c->cap_c3_valid = c->cap_search_valid = false;
  int rc = c3h_set_grid(c, grids[0], k.div_b, k.min_b, k.leaf, 1);
  if (rc == C3H_OK) rc = extract_frames(c, grids, nb, &k.p, nullptr, nullptr);
  if (rc == C3H_OK) rc = search_frames(c, nb, k.range, k.thr, k.rotate, outs, 2);
  c->capture = false;
  c->cap_q.lim = lim;  // canvas frames: each frame's own subdivisions bound its positions
  c->cap_q.score_engine = ctx->score_engine;  // the tick's score role (launch_tick)
  if (rc < 0) {
    if (c != ctx) ctx->err = c->err;
    return rc;
  }
  // points-in frames without subdivisions (S = 0, one histogram): the reference runs no search
  // (search_frames returned 0: setData returns early), the batch is its C3 stage alone
  if (rc == 0 && lim && k.p.subdiv == 0 && c->cap_c3_valid && c3h::tick_ok(c->cap_c3)) {
    c->nframes_feat = 1;
    *fresh = c3h_ctx::PipeBatch{c->cap_c3, c3h::SparseSearch{}, c3h::SparseCompress{}, nb, 0};
    fresh->nosearch = true;
    return 1;
  }
  *fresh = c3h_ctx::PipeBatch{c->cap_c3, c->cap_q, c->cap_sc, nb, 0};
  const bool fits = c->cap_c3_valid && c->cap_search_valid && c->cap_sparse_g && c3h::tick_ok(c->cap_c3) &&
                    pipe_capture_end(ctx, c, k.range, outs, nb, fresh);
  if (!fits) {  // one geometry per stream: decided on its first batch
    if (!ctx->pipe.empty()) return fail(ctx, C3H_ERR_STATE, "pipeline: internal: geometry changed");
    return 0;
  }
  c->nframes_feat = 1;  // slot 0 is the context's view from here on
  return rc;
}

// Launches a prepared batch's first tick; rc: pipe_prepare's result (> 0)
int pipe_commit(c3h_ctx* ctx, const c3h_ctx::PipeBatch& fresh, const c3h_ctx::PipeKey& k, int rc) {
  if (ctx->pipe.empty()) {
    // a stream starts: the occupancy role's tail-stealing pool (words 0-1 of each buffer
    // set's tile flags) resets itself at the end of every launch; zero it here as well, so
    // a launch that ended early (an aborted stream) cannot leave it counting
    for (int sidx = 0; sidx < kPipeDepth; ++sidx) {
      c3h_ctx* c = sidx == 0 ? ctx : (sidx - 1 < (int)ctx->lanes.size() ? ctx->lanes[sidx - 1] : nullptr);
      if (c && c->tileflags.p && c->tileflags.n >= 2)
        HIPCHK(hipMemsetAsync(c->tileflags.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    }
  }
  int trc = pipe_tick(ctx, &fresh);
  if (trc != C3H_OK) return trc;
  ctx->pipe_seq++;
  ctx->pipe_key = k;
  ctx->pipe_nm = rc;
  return rc;
}

// the key fields of every kind of stream: the grid (or canvas) dims, the search and the batch
void key_base(const c3h_ctx* ctx, const int32_t div_b[3], const int32_t range[3], int32_t thr, int32_t rotate, int B,
              c3h_ctx::PipeKey* k) {
  memcpy(k->div_b, div_b, sizeof(k->div_b));
  memcpy(k->range, range, sizeof(k->range));
  k->thr = thr;
  k->rotate = rotate ? 1 : 0;
  k->batch = B;
  k->rank = ctx->rank;
  k->remove_overlap = ctx->remove_overlap;
  k->setup_version = ctx->setup_version;
}

c3h_ctx::PipeKey pipe_key(c3h_ctx* ctx, const int32_t div_b[3], const int32_t min_b[3], float leaf,
                          const c3h_extract_params* p, const int32_t range[3], int32_t thr, int32_t rotate,
                          int B) {
  c3h_ctx::PipeKey k;
  memset(&k, 0, sizeof(k));  // compared bytewise
  key_base(ctx, div_b, range, thr, rotate, B, &k);
  memcpy(k.min_b, min_b, sizeof(k.min_b));
  k.leaf = leaf;
  k.p = *p;
  return k;
}

// models the tick's score role takes: r <= 64 (either engine), or wide ones on the matrix
// cores (with c3h_set_score_engine(1) there is no VALU role for them: the lanes)
bool tick_models_ok(const c3h_ctx* ctx) {
  return c3h::score_fast_ok(ctx->D, ctx->r) ||
         (ctx->score_engine != 1 && c3h::score_tick_wide_ok(ctx->D, ctx->M, ctx->r));
}

bool pipelinable(const c3h_ctx* ctx) {
  return ctx->pipeline && ctx->rank >= 1 && ctx->rank <= 64 && tick_models_ok(ctx);
}

// Runs nframes of the stream k through the pipeline in batches of B.  prepare(frame_idx, nb,
// fresh) captures the frames frame_idx[0 .. nb) as the next batch on its buffer set and returns
// as pipe_prepare; its first tick is launched here.  drain: run the fill/drain ticks so every
// result is complete on return (c3h_run_frames); the last batch is then placed on set 0 with
// its last frame in slot 0, so this context holds the last frame's state.
// Returns > 0 (modes searched), 0 when the first batch does not fit the tick (nothing was
// launched: the caller takes another route), < 0 on error.
template <class Prepare>
int pipe_run(c3h_ctx* ctx, const c3h_ctx::PipeKey& k, int nframes, int B, bool drain, Prepare&& prepare) {
  int rc = ensure_lanes(ctx, kPipeDepth - 1);
  if (rc == C3H_OK && !ctx->pipe.empty() && memcmp(&k, &ctx->pipe_key, sizeof(k)) != 0)
    rc = pipe_flush(ctx);  // a different stream: drain the open one first
  if (rc != C3H_OK) return rc;
  PipeScope scope(ctx);
  const int nchunks = c3h::chunk_count(nframes, B);
  if (drain && ctx->pipe.empty()) ctx->pipe_seq = c3h::drain_start_seq(nchunks);  // the last batch lands on set 0
  int nm = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    int frame_idx[c3h::kMaxBatch];
    const int nb = c3h::chunk_size(nframes, B, ch);
    for (int j = 0; j < nb; ++j) frame_idx[j] = c3h::chunk_frame(nframes, B, ch, j, drain);
    c3h_ctx::PipeBatch fresh{};
    rc = prepare(frame_idx, nb, &fresh);
    if (rc > 0) rc = pipe_commit(ctx, fresh, k, rc);
    if (rc <= 0) {
      if (rc == 0 && ch == 0) return 0;
      ctx->pipe.clear();
      return rc == 0 ? fail(ctx, C3H_ERR_STATE, "pipeline: internal: batch does not fit") : rc;
    }
    nm = rc;
  }
  if (drain) rc = pipe_drain(ctx);
  return rc < 0 ? rc : nm;
}

// c3h_run_frames (drain) / c3h_stream_frames through the pipeline.  Returns as pipe_run.
int run_frames_pipelined(c3h_ctx* ctx, const uint32_t* const* d_grids, int32_t nframes,
                         const int32_t div_b[3], const int32_t min_b[3], float leaf,
                         const c3h_extract_params* p, const int32_t range[3], int32_t exist_threshold,
                         int32_t rotate, c3h_det* d_out, int B, bool drain) {
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  const c3h_ctx::PipeKey k = pipe_key(ctx, div_b, min_b, leaf, p, range, exist_threshold, rotate, B);
  return pipe_run(ctx, k, nframes, B, drain, [&](const int* frame_idx, int nb, c3h_ctx::PipeBatch* fresh) {
    const uint32_t* grids[c3h::kMaxBatch];
    c3h_det* outs[c3h::kMaxBatch];
    for (int j = 0; j < nb; ++j) {
      grids[j] = d_grids[frame_idx[j]];
      outs[j] = d_out + (size_t)frame_idx[j] * per_frame;
    }
    return pipe_prepare(ctx, grids, outs, nb, k, nullptr, fresh);
  });
}

}  // namespace

extern "C" {

int c3h_run_frames(c3h_ctx* ctx, const uint32_t* const* d_grids, int32_t nframes,
                   const int32_t div_b[3], const int32_t min_b[3], float leaf,
                   const c3h_extract_params* p, const int32_t range[3], int32_t exist_threshold,
                   int32_t rotate, c3h_det* d_out) {
  if (!ctx || !d_grids || nframes < 0 || !div_b || !min_b || !p || !range || !d_out)
    return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, "c3h_run_frames: no axes (call c3h_search_setup)");
  if (!extract_params_ok(p)) return fail(ctx, C3H_ERR_ARG, "c3h_run_frames: variant / color_mode");
  if (int rc = overlap_rank_check(ctx, "c3h_run_frames")) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = pipe_flush(ctx)) return rc;  // an open stream completes first
  if (nframes == 0) return 0;
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  // frames go in chunks of B (one set of launches per chunk, frame = launch y / z index)
  const int Bset = std::max(1, std::min(ctx->nbatch, c3h::kMaxBatch));
  if (pipelinable(ctx)) {
    const int rc = run_frames_pipelined(ctx, d_grids, nframes, div_b, min_b, leaf, p, range, exist_threshold,
                                        rotate, d_out, Bset, true);
    if (rc != 0) return rc;
  }
  // the lanes' multi-frame launch is the VALU list kernel's: wide models (r > 64) go one frame
  // per chunk there, whatever batch the pipeline was offered
  const int B = c3h::score_fast_ok(ctx->D, ctx->r) ? Bset : 1;
  const int nchunks = (nframes + B - 1) / B;
  // lanes: chunks are spread over K child contexts on their own streams and host threads
  const int K = std::max(1, std::min(ctx->nlanes, nchunks));
  if (int rc = ensure_lanes(ctx, K - 1)) return rc;
  if (!ctx->fork_ev) HIPCHK(hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(ctx->fork_ev, ctx->stream));  // inputs were produced on ctx's stream
  for (int l = 0; l < K - 1; ++l) HIPCHK(hipStreamWaitEvent(ctx->lanes[l]->stream, ctx->fork_ev, 0));
  std::vector<int> lane_rc(K, 0);
  auto run_lane = [&](int lane) {
    c3h_ctx* c = lane == 0 ? ctx : ctx->lanes[lane - 1];
    if (lane) (void)hipSetDevice(c->device);
    int nm_lane = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
      if ((nchunks - 1 - ch) % K != lane) continue;
      const uint32_t* grids[c3h::kMaxBatch];
      c3h_det* outs[c3h::kMaxBatch];
      const int nb = c3h::chunk_size(nframes, B, ch);
      for (int j = 0; j < nb; ++j) {  // the lane that runs the last chunk ends up holding the last frame's state
        const int fi = c3h::chunk_frame(nframes, B, ch, j, true);
        grids[j] = d_grids[fi];
        outs[j] = d_out + (size_t)fi * per_frame;
      }
      int rc = c3h_set_grid(c, grids[0], div_b, min_b, leaf, 1);
      if (rc == C3H_OK) rc = extract_frames(c, grids, nb, p, nullptr, nullptr);
      if (rc == C3H_OK) rc = search_frames(c, nb, range, exist_threshold, rotate, outs, 2);
      rc = overlap_behind(ctx, c, range, outs, nb, rc);
      if (rc < 0) {
        lane_rc[lane] = rc;
        return;
      }
      nm_lane = rc;
      c->nframes_feat = 1;  // slot 0 is the context's view from here on
    }
    lane_rc[lane] = nm_lane;
  };
  std::vector<std::thread> workers;
  for (int l = 1; l < K; ++l) workers.emplace_back(run_lane, l);
  run_lane(0);
  for (auto& w : workers) w.join();
  for (int l = 1; l < K; ++l)
    if (lane_rc[l] < 0) return fail(ctx, lane_rc[l], std::string("c3h_run_frames lane: ") + ctx->lanes[l - 1]->err);
  if (lane_rc[0] < 0) return lane_rc[0];
  for (int l = 0; l < K - 1; ++l) {  // join
    HIPCHK(hipEventRecord(ctx->lane_ev[l], ctx->lanes[l]->stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->lane_ev[l], 0));
  }
  return lane_rc[0];
}

int c3h_stream_frames(c3h_ctx* ctx, const uint32_t* const* d_grids, int32_t nframes,
                      const int32_t div_b[3], const int32_t min_b[3], float leaf,
                      const c3h_extract_params* p, const int32_t range[3], int32_t exist_threshold,
                      int32_t rotate, c3h_det* d_out) {
  if (!ctx || !d_grids || nframes < 0 || !div_b || !min_b || !p || !range || !d_out)
    return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, "c3h_stream_frames: no axes (call c3h_search_setup)");
  if (!extract_params_ok(p)) return fail(ctx, C3H_ERR_ARG, "c3h_stream_frames: variant / color_mode");
  if (int rc = overlap_rank_check(ctx, "c3h_stream_frames")) return rc;
  if (nframes == 0) return ctx->pipe_nm;
  HIPCHK(hipSetDevice(ctx->device));
  const int B = std::max(1, std::min(ctx->nbatch, c3h::kMaxBatch));
  if (pipelinable(ctx)) {
    const int rc = run_frames_pipelined(ctx, d_grids, nframes, div_b, min_b, leaf, p, range, exist_threshold,
                                        rotate, d_out, B, false);
    if (rc != 0) return rc;
  }
  // not pipelinable: the frames complete as in c3h_run_frames
  return c3h_run_frames(ctx, d_grids, nframes, div_b, min_b, leaf, p, range, exist_threshold, rotate, d_out);
}

int c3h_stream_flush(c3h_ctx* ctx) {
  if (!ctx) return C3H_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  return pipe_flush(ctx);
}

}  // extern "C"

namespace {

// ---- feature-rows batches (c3h_run_feature_frames) -------------------------------------
// A batch of caller-computed rows enters the pipeline at the compress + gate slot: its front
// kernel (feat_front.hip), one launch ahead of the batch's first tick, writes the buffer set's
// exist values, has-data words, row list and feature rows on the canvas layout, which is all
// the tick's later roles read of an extract.

// the buffer set's state and buffers for nb frames of `dim` floats on a canvas of H rows: an
// extract of nb frames whose non-empty rows are listed
int feature_set_state(c3h_ctx* ctx, int nb, int64_t H, int dim, const int32_t canvas[3]) {
  ctx->have_feat = false;
  ctx->feat16_pending = false;
  ctx->g_valid = false;
  ctx->g_sparse = false;
  ctx->feat_sparse = false;
  ctx->exist_gates_rows = false;
  ENSURE(ctx->feat, (size_t)nb * H * dim);
  ENSURE(ctx->exist, (size_t)nb * H);
  ENSURE(ctx->rows, (size_t)nb * H);
  ENSURE(ctx->ff_has, (size_t)nb * H);
  ENSURE(ctx->ff_cnt, (size_t)c3h::kMaxBatch);
  ENSURE(ctx->ff_lim, (size_t)c3h::kMaxBatch * 4);
  ctx->hist_num = H;
  ctx->feat_dim = dim;
  for (int a = 0; a < 3; ++a) ctx->subdiv_b[a] = canvas[a];
  ctx->nframes_feat = nb;
  ctx->rows_valid = true;
  ctx->feat_listed = true;
  ctx->have_feat = true;
  return C3H_OK;
}

// Captures nb frames of rows as the next batch on its buffer set and enqueues its front
// kernel.  Returns as pipe_prepare: > 0 modes searched, 0 when the configuration does not fit
// the tick (nothing was enqueued), < 0 on error.
int feature_prepare(c3h_ctx* ctx, const float* const* feats, const int32_t* const* exists,
                    const int32_t* const* sbs, c3h_det* const* outs, int nb, const c3h_ctx::PipeKey& k,
                    c3h_ctx::PipeBatch* fresh) {
  c3h_ctx* c = pipe_set(ctx, ctx->pipe_seq);
  const int64_t H = (int64_t)k.div_b[0] * k.div_b[1] * k.div_b[2];
  int rc = feature_set_state(c, nb, H, k.dim, k.div_b);
  if (rc == C3H_OK) {
    c->capture = true;
    c->cap_c3_valid = c->cap_search_valid = false;
    rc = search_frames(c, nb, k.range, k.thr, k.rotate, outs, 2);
    c->capture = false;
  }
  if (rc < 0) {
    c->have_feat = false;
    if (c != ctx) ctx->err = c->err;
    return rc;
  }
  *fresh = c3h_ctx::PipeBatch{c3h::C3Launch{}, c->cap_q, c->cap_sc, nb, 0};
  if (!(rc > 0 && c->cap_search_valid && c->cap_sparse_g &&
        pipe_capture_end(ctx, c, k.range, outs, nb, fresh))) {  // one geometry per stream
    c->have_feat = false;
    if (!ctx->pipe.empty()) return fail(ctx, C3H_ERR_STATE, "pipeline: internal: geometry changed");
    return 0;
  }
  c->nframes_feat = 1;  // slot 0 is the context's view from here on
  c3h::FeatFront ff{};
  for (int j = 0; j < nb; ++j) {
    ff.feat[j] = feats[j];
    ff.exist_in[j] = exists ? exists[j] : nullptr;
    for (int a = 0; a < 3; ++a) ff.sb[j][a] = sbs[j][a];
  }
  ff.nf = nb;
  ff.dim = k.dim;
  ff.rule = k.rule < 0 ? 0 : k.rule;
  ff.R = c3h::fr_block_rows(k.dim);
  ff.magic = c3h::fr_div_magic(k.dim);
  for (int a = 0; a < 3; ++a) ff.cb[a] = k.div_b[a];
  ff.out = c->feat.p;
  ff.exist = c->exist.p;
  ff.has = c->ff_has.p;
  ff.rows = c->rows.p;
  ff.cnt = c->ff_cnt.p;
  ff.lim = c->ff_lim.p;
  ff.s_out = H * k.dim;
  ff.s_h = H;
  // (the set's previous batch left the pipeline two batches ago: stream order covers its reads)
  HIPCHK(hipMemsetAsync(c->ff_cnt.p, 0, (size_t)c3h::kMaxBatch * sizeof(uint32_t), ctx->stream));
  {
    Timed t(ctx, 1, nb);
    HIPCHK(c3h::launch_feat_front(ff, ctx->stream));
  }
  fresh->rows_in = true;
  // the gate role: the true exist values, positions bounded by each frame's own counts
  fresh->q.lim = c->ff_lim.p;
  fresh->q.score_engine = ctx->score_engine;
  // the compress role: the front kernel's list (its counters in place of the extract's)
  fresh->sc.nrows = c->ff_cnt.p;
  fresh->sc.s_nrows = 1;
  // the score role skips rows by the has-data words: exist 0 does not mean an empty row here
  fresh->qs = fresh->q;
  fresh->qs.exist = c->ff_has.p;
  fresh->qs.skip_empty = 1;
  return rc;
}

c3h_ctx::PipeKey feature_key(c3h_ctx* ctx, const int32_t canvas[3], int dim, int rule, const int32_t range[3],
                             int32_t thr, int32_t rotate, int B) {
  c3h_ctx::PipeKey k;
  memset(&k, 0, sizeof(k));  // compared bytewise
  key_base(ctx, canvas, range, thr, rotate, B, &k);
  k.rows_in = 1;
  k.dim = dim;
  k.rule = rule;  // -1: the caller's exist arrays
  return k;
}

// c3h_run_feature_frames (drain) / c3h_stream_feature_frames through the pipeline.  Returns as
// pipe_run (0: nothing was enqueued).
int feature_frames_pipelined(c3h_ctx* ctx, const float* const* d_feat, const int32_t* const* d_exist,
                             int32_t nframes, const int32_t* subdiv_b, const int32_t canvas[3], int dim,
                             int rule, const int32_t range[3], int32_t thr, int32_t rotate, c3h_det* d_out,
                             int B, bool drain) {
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  const c3h_ctx::PipeKey k = feature_key(ctx, canvas, dim, d_exist ? -1 : rule, range, thr, rotate, B);
  return pipe_run(ctx, k, nframes, B, drain, [&](const int* frame_idx, int nb, c3h_ctx::PipeBatch* fresh) {
    const float* feats[c3h::kMaxBatch];
    const int32_t* exists[c3h::kMaxBatch];
    const int32_t* sbs[c3h::kMaxBatch];
    c3h_det* outs[c3h::kMaxBatch];
    for (int j = 0; j < nb; ++j) {
      const int fi = frame_idx[j];
      feats[j] = d_feat[fi];
      exists[j] = d_exist ? d_exist[fi] : nullptr;
      sbs[j] = subdiv_b + 3 * fi;
      outs[j] = d_out + (size_t)fi * per_frame;
    }
    return feature_prepare(ctx, feats, d_exist ? exists : nullptr, sbs, outs, nb, k, fresh);
  });
}

int feature_frames(c3h_ctx* ctx, const float* const* d_feat, const int32_t* const* d_exist, int32_t nframes,
                   const int32_t* subdiv_b, const int32_t canvas_b[3], int32_t dim, int32_t exist_rule,
                   const int32_t range[3], int32_t thr, int32_t rotate, c3h_det* d_out, bool stream) {
  const char* who = stream ? "c3h_stream_feature_frames" : "c3h_run_feature_frames";
  if (!ctx || !d_feat || nframes < 0 || (nframes > 0 && !subdiv_b) || !canvas_b || !range || !d_out || dim <= 0)
    return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, std::string(who) + ": no axes (call c3h_search_setup)");
  if (!d_exist && (exist_rule < 0 || exist_rule > 2)) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": exist rule");
  if (!d_exist && dim < c3h::fr_exist_min_dim(exist_rule))
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": the exist rule needs more columns (VOSCH 22, GRSD 20, C3-HLAC 2)");
  if (dim != ctx->F) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": feature dimension differs from the scene axis");
  if (range[0] < 1 || range[1] < 1 || range[2] < 1) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": ranges must be >= 1");
  if (int rc = overlap_rank_check(ctx, who)) return rc;
  int64_t H = 1;
  for (int a = 0; a < 3; ++a) {
    if (canvas_b[a] < 0) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": canvas_b");
    H *= canvas_b[a];
  }
  if (H > INT32_MAX) return fail(ctx, C3H_ERR_RANGE, std::string(who) + ": canvas beyond int32 row indices");
  for (int i = 0; i < nframes; ++i) {
    int64_t h = 1;
    for (int a = 0; a < 3; ++a) {
      const int32_t n = subdiv_b[3 * i + a];
      if (n < 0 || n > canvas_b[a]) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": a frame's subdiv_b exceeds canvas_b");
      h *= n;
    }
    if (h > 0 && (!d_feat[i] || ((uintptr_t)d_feat[i] & 3) || (d_exist && (!d_exist[i] || ((uintptr_t)d_exist[i] & 3)))))
      return fail(ctx, C3H_ERR_ARG, std::string(who) + ": frame pointers must be device pointers aligned to 4 bytes");
  }
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = stream ? C3H_OK : pipe_flush(ctx)) return rc;  // an open stream completes first
  int modes[6];
  const int nm_sched = mode_schedule(range[0], range[1], range[2], rotate, modes);
  if (nframes == 0) return stream ? ctx->pipe_nm : 0;
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  const int B = std::max(1, std::min(ctx->nbatch, c3h::kMaxBatch));
  if (H > 0 && pipelinable(ctx) && c3h::feat_front_ok(dim)) {
    const int rc = feature_frames_pipelined(ctx, d_feat, d_exist, nframes, subdiv_b, canvas_b, dim, exist_rule, range,
                                            thr, rotate, d_out, B, !stream);
    if (rc != 0) return rc;
  }
  // Routes the tick does not take (c3h_set_pipeline(0), rank > 64, models or axes it has no
  // role for): frame by frame as a caller would, c3h_set_features + a search from the setRank
  // state into the frame's slot, in the frame's own layout
  if (int rc = pipe_flush(ctx)) return rc;
  for (int i = 0; i < nframes; ++i) {
    c3h_det* out = d_out + (size_t)i * per_frame;
    int rc = c3h_set_features(ctx, d_feat[i], subdiv_b + 3 * i, dim, d_exist ? d_exist[i] : nullptr, exist_rule, 1);
    if (rc == C3H_OK) rc = c3h_set_rank(ctx, ctx->rank);
    if (rc == C3H_OK) rc = c3h_search_async(ctx, range, thr, rotate, out);
    rc = overlap_behind(ctx, ctx, range, &out, 1, rc);
    if (rc < 0) return rc;
  }
  return nm_sched;
}

}  // namespace

extern "C" {

int c3h_run_feature_frames(c3h_ctx* ctx, const float* const* d_feat, const int32_t* const* d_exist,
                           int32_t nframes, const int32_t* subdiv_b, const int32_t canvas_b[3], int32_t dim,
                           int32_t exist_rule, const int32_t range[3], int32_t exist_threshold, int32_t rotate,
                           c3h_det* d_out) {
  return feature_frames(ctx, d_feat, d_exist, nframes, subdiv_b, canvas_b, dim, exist_rule, range, exist_threshold,
                        rotate, d_out, false);
}

int c3h_stream_feature_frames(c3h_ctx* ctx, const float* const* d_feat, const int32_t* const* d_exist,
                              int32_t nframes, const int32_t* subdiv_b, const int32_t canvas_b[3], int32_t dim,
                              int32_t exist_rule, const int32_t range[3], int32_t exist_threshold, int32_t rotate,
                              c3h_det* d_out) {
  return feature_frames(ctx, d_feat, d_exist, nframes, subdiv_b, canvas_b, dim, exist_rule, range, exist_threshold,
                        rotate, d_out, true);
}

}  // extern "C"

namespace {

// One frame on the single-frame path (c3h_voxelize + c3h_extract + search from the setRank
// state) into d_out_f: the frames c3h_run_point_frames' canvas cannot reproduce exactly.
int point_frame_single(c3h_ctx* ctx, const float* pts, int64_t n, int on_device, float leaf, float z_limit,
                       const c3h_extract_params* p, const int32_t range[3], int32_t thr, int32_t rotate,
                       c3h_det* d_out_f, c3h_frame_info* fi) {
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  HIPCHK(hipMemsetAsync(d_out_f, 0, per_frame * sizeof(c3h_det), ctx->stream));  // fresh lists
  c3h_grid_info gi{};
  int rc = c3h_voxelize(ctx, pts, n, on_device, leaf, z_limit, &gi);
  int32_t sb[3] = {0, 0, 0};
  if (rc == C3H_OK) rc = extract_frames(ctx, &ctx->grid_ptr, 1, p, sb, nullptr);
  if (rc == C3H_OK) rc = search_frames(ctx, 1, range, thr, rotate, &d_out_f, 2);
  rc = overlap_behind(ctx, ctx, range, &d_out_f, 1, rc);
  if (fi) {
    memset(fi, 0, sizeof(*fi));
    if (rc >= 0) {
      for (int a = 0; a < 3; ++a) {
        fi->div_b[a] = gi.div_b[a];
        fi->min_b[a] = gi.min_b[a];
        fi->subdiv_b[a] = sb[a];
      }
      fi->n_valid = gi.n_valid;
      fi->n_occ = gi.n_occ;
    }
    fi->status = rc >= 0 ? 1 : rc;
  }
  return rc < 0 ? rc : C3H_OK;
}

// Where the frames of a points-in call come from: packed x y z rgb float arrays
// (c3h_run_point_frames) or sensor_msgs/PointCloud2 messages the batched voxeliser reads in
// place (c3h_run_pointcloud2_frames: layout != nullptr).  base[i] is frame i's pts[i] or
// data[i], n[i] its points.
struct PointSrc {
  std::string who;
  const void* const* base = nullptr;
  const int64_t* n = nullptr;
  int32_t nframes = 0;
  int on_device = 0;
  const c3h_pc2_layout* layout = nullptr;
  const uint32_t *height = nullptr, *width = nullptr, *row_step = nullptr;
  c3h::Pc2Plan plan{};
  // the bytes of frame i (what a host frame's staging copy moves)
  size_t bytes(int i) const {
    return layout ? (size_t)c3h::pc2_msg_bytes(height[i], width[i], layout->point_step, row_step[i]) : (size_t)n[i] * 16;
  }
  // the batch's staging buffer: frames follow each other at 16-byte aligned offsets
  static size_t staged(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
};

// Frame i on the single-frame path.  A message is converted by the single-frame path's own
// converter into the context's point buffer first (c3h_voxelize_pointcloud2's steps).
int point_src_single(c3h_ctx* ctx, const PointSrc& s, int i, float leaf, float z_limit, const c3h_extract_params* p,
                     const int32_t range[3], int32_t thr, int32_t rotate, c3h_det* d_out_f, c3h_frame_info* fi) {
  if (!s.layout)
    return point_frame_single(ctx, static_cast<const float*>(s.base[i]), s.n[i], s.on_device, leaf, z_limit, p, range,
                              thr, rotate, d_out_f, fi);
  const void* msg = s.base[i];
  const size_t bytes = s.bytes(i);
  if (bytes > 0 && !s.on_device) {
    ENSURE(ctx->raw, (bytes + 3) / 4);
    HIPCHK(hipMemcpyAsync(ctx->raw.p, msg, bytes, hipMemcpyHostToDevice, ctx->stream));
    msg = ctx->raw.p;
  }
  ENSURE(ctx->pts, (size_t)std::max<int64_t>(s.n[i], 1) * 4);
  const uint32_t ps = s.layout->point_step;
  HIPCHK(c3h::launch_pc2_convert(msg, s.height[i], s.width[i], ps, s.height[i] > 1 ? s.row_step[i] : s.width[i] * ps,
                                 s.layout->offsets, s.layout->is_bigendian ? 1 : 0, ctx->pts.p, ctx->stream));
  return point_frame_single(ctx, ctx->pts.p, s.n[i], 1, leaf, z_limit, p, range, thr, rotate, d_out_f, fi);
}

// One points-in call on the pipeline: what its batches share, and the steps run_point_source
// sequences around the voxeliser stream's launches and events.
struct PointCall {
  c3h_ctx* ctx;
  const PointSrc& src;
  float leaf, z_limit;
  const int32_t* canvas;
  const c3h_extract_params* p;
  int64_t cvox;  // canvas voxels
  int B;         // frames per batch
  int chunk;     // points per accumulate block
  // toroidal accumulator dims: powers of two >= the canvas (a frame whose extent fits the
  // canvas never wraps onto itself; the index is then three masks and shifts)
  int tb[3] = {0, 0, 0};
  int64_t tvox = 1;

  // The buffers every batch of the call shares -- toroidal accumulators (one per frame slot; the
  // scatter returns them to zero), voxel lists, the frames' records, host staging -- sized, and
  // zeroed on the context's stream, before the first batch; the voxeliser's stream and the events.
  int shared_setup() {
    const int nchunks = c3h::chunk_count(src.nframes, B);
    for (int a = 0; a < 3; ++a) {
      tb[a] = 0;
      while ((1 << tb[a]) < canvas[a]) ++tb[a];
      tvox <<= tb[a];
    }
    if (tvox > ((int64_t)1 << 31)) return fail(ctx, C3H_ERR_RANGE, src.who + ": canvas too large");
    if (ctx->pb_acc_vox != tvox || ctx->pb_acc_slots < B) {
      ENSURE(ctx->pb_acc, (size_t)B * tvox);
      ENSURE(ctx->pb_accM, (size_t)B * tvox);
      ENSURE(ctx->pb_fcnt, (size_t)c3h::kMaxBatch);
      HIPCHK(hipMemsetAsync(ctx->pb_acc.p, 0, (size_t)B * tvox * 16, ctx->stream));
      HIPCHK(hipMemsetAsync(ctx->pb_accM.p, 0xff, (size_t)B * tvox * 4, ctx->stream));
      HIPCHK(hipMemsetAsync(ctx->pb_fcnt.p, 0, (size_t)c3h::kMaxBatch * 4, ctx->stream));
      ctx->pb_acc_vox = tvox;
      ctx->pb_acc_slots = B;
    }
    ENSURE(ctx->pb_info, (size_t)src.nframes);
    // shared buffers sized for the largest batch up front: the voxeliser stream may still be
    // reading them while the next batch is prepared
    {
      int64_t max_blk = 1;
      size_t max_bytes = 16;
      for (int ch = 0; ch < nchunks; ++ch) {
        int64_t b = 0;
        size_t q = 0;
        for (int j = ch * B; j < std::min(src.nframes, (ch + 1) * B); ++j) {
          b += std::max<int64_t>(1, (src.n[j] + chunk - 1) / chunk);
          q += PointSrc::staged(src.bytes(j));
        }
        max_blk = std::max(max_blk, b);
        max_bytes = std::max(max_bytes, q);
      }
      if (max_blk > INT_MAX / chunk) return fail(ctx, C3H_ERR_RANGE, src.who + ": batch too large");
      ENSURE(ctx->pb_vlist, (size_t)max_blk * chunk);
      if (!src.on_device) {  // the messages' raw bytes have a byte buffer of their own
        if (src.layout) ENSURE(ctx->pb_raw, max_bytes);
        else ENSURE(ctx->pb_stage, max_bytes / 4);
      }
    }
    if (!ctx->pb_vstream) {
      // the voxeliser's stream is the points-in call's critical path (its accumulate runs
      // beside the tick of the batches before, which has slack): high priority, so its
      // workgroups are dispatched first as CUs free up
      int lo = 0, hi = 0;
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
        HIPCHK(hipStreamCreateWithPriority(&ctx->pb_vstream, hipStreamNonBlocking, hi));
      else
        HIPCHK(hipStreamCreateWithFlags(&ctx->pb_vstream, hipStreamNonBlocking));
    }
    if (!ctx->pb_vox_ev) HIPCHK(hipEventCreateWithFlags(&ctx->pb_vox_ev, hipEventDisableTiming));
    for (hipEvent_t& e : ctx->pb_tick_ev)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return C3H_OK;
  }

  // Buffer set c holds `total` accumulate blocks of B frames on this canvas.  A reallocation
  // loses the previous batch's word lists, so the canvas grids are then zeroed whole.
  int set_buffers(c3h_ctx* c, int total, hipStream_t vs) {
    const int blk_cap = (int)std::min<int64_t>(c->pb_part.n / c3h::vox_part_words(), INT_MAX);
    if (c->pb_cvox != cvox || c->pb_slots < B || blk_cap < total) {
      // (re)allocation: nothing in flight may still use the set's old buffers
      HIPCHK(hipStreamSynchronize(vs));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      const int bc = std::max(total, blk_cap);
      ENSURE(c->pb_grid, (size_t)B * cvox);
      ENSURE(c->pb_lim, (size_t)B * 4);
      ENSURE(c->pb_part, (size_t)bc * c3h::vox_part_words());
      ENSURE(c->pb_wlist, (size_t)bc * chunk);
      ENSURE(c->pb_flags, (size_t)B * c3h::kVbFlagCap);
      ENSURE(c->pb_bucket, (size_t)B * c3h::kVbBucketCap);
      ENSURE(c->pb_moved, (size_t)B * c3h::kVbMovedCap);
      ENSURE(c->pb_xcnt, (size_t)B * 4);
      HIPCHK(hipMemsetAsync(c->pb_grid.p, 0, (size_t)B * cvox * 4, vs));
      c->pb_cvox = cvox;
      c->pb_slots = B;
      c->pb_prev_total = 0;
      c->pb_prev_nf = 0;
    }
    return C3H_OK;
  }

  // The voxeliser's arguments for the frames f0 .. f0 + nb - 1 as the next batch on buffer set c
  // (all but what the batch's C3 launch supplies: launch_args).  Host frames' staging copies are
  // enqueued on vs.
  int vox_args(c3h_ctx* c, int f0, int nb, hipStream_t vs, c3h::VoxBatchArgs& va) {
    va.nf = nb;
    va.blk0[0] = 0;
    for (int j = 0; j < nb; ++j) {  // every frame at least one block: it publishes the record
      va.n[j] = src.n[f0 + j];
      va.blk0[j + 1] = va.blk0[j] + (int)std::max<int64_t>(1, (src.n[f0 + j] + chunk - 1) / chunk);
    }
    va.total = va.blk0[nb];
    if (int rc = set_buffers(c, va.total, vs)) return rc;
    va.prev_nf = c->pb_prev_nf;
    va.prev_total = c->pb_prev_total;
    for (int j = 0; j <= c3h::kMaxBatch; ++j)
      va.prev_blk0[j] = j < (int)c->pb_prev_blk0.size() ? c->pb_prev_blk0[j] : va.prev_total;
    if (src.on_device) {
      for (int j = 0; j < nb; ++j) va.pts[j] = static_cast<const float4*>(src.base[f0 + j]);
    } else {  // host frames: one staging copy per batch, ordered on the voxeliser stream
      uint8_t* stage = src.layout ? ctx->pb_raw.p : reinterpret_cast<uint8_t*>(ctx->pb_stage.p);
      size_t o = 0;
      for (int j = 0; j < nb; ++j) {
        va.pts[j] = reinterpret_cast<const float4*>(stage + o);
        const size_t bytes = src.bytes(f0 + j);
        if (bytes > 0) HIPCHK(hipMemcpyAsync(stage + o, src.base[f0 + j], bytes, hipMemcpyHostToDevice, vs));
        o += PointSrc::staged(bytes);
      }
    }
    if (src.layout) {  // the voxeliser reads the messages in place
      va.src = 1;
      va.pc2 = src.plan;
      for (int j = 0; j < nb; ++j) {
        const c3h::Pc2Frame fr =
            c3h::pc2_frame(src.height[f0 + j], src.width[f0 + j], src.layout->point_step, src.row_step[f0 + j]);
        va.pc2_width[j] = fr.width;
        va.pc2_row_step[j] = fr.row_step;
        va.pc2_magic[j] = fr.magic;
        va.pc2_shift[j] = (uint8_t)fr.shift;
      }
    }
    va.inv = 1.0f / leaf;
    va.leaf = leaf;
    va.z_limit = z_limit;
    for (int a = 0; a < 3; ++a) {
      va.C[a] = canvas[a];
      va.off[a] = p->subdiv > 0 ? p->offset[a] : 0;
    }
    va.subdiv = p->subdiv;
    va.inv_s = p->subdiv > 0 ? (float)(1.0 / p->subdiv) : 0.0f;
    for (int a = 0; a < 3; ++a) va.tb[a] = tb[a];
    va.acc = ctx->pb_acc.p;
    va.accM = ctx->pb_accM.p;
    va.s_acc = tvox;
    va.fcnt = ctx->pb_fcnt.p;
    va.vlist = ctx->pb_vlist.p;
    va.wlist = c->pb_wlist.p;
    va.part = c->pb_part.p;
    // every slot of the set: the previous batch on it may have had more frames than this one
    for (int j = 0; j < c3h::kMaxBatch; ++j)
      va.grid[j] = j < c->pb_slots ? c->pb_grid.p + (size_t)j * cvox : nullptr;
    if (va.prev_nf > c->pb_slots || va.nf > c->pb_slots)
      return fail(ctx, C3H_ERR_STATE, src.who + ": internal: frame slots");
    va.info = ctx->pb_info.p + f0;
    va.lim = c->pb_lim.p;
    return C3H_OK;
  }

  // ... and what the scatter takes of the batch's captured C3 launch: the tile stamps and work
  // lists it writes in the occupancy stream's place
  void launch_args(const c3h::C3Launch& cl, c3h::VoxBatchArgs& va) const {
    va.stamp = (cl.gx == canvas[0] && cl.gy == canvas[1] && cl.gz == canvas[2] &&
                cl.ntiles <= ((int64_t)1 << 18)) ? 1 : 0;
    va.axmap = cl.axmap;
    va.ns0 = cl.nseg[0];
    va.ns1 = cl.nseg[1];
    va.ntiles = (int)cl.ntiles;
    va.epoch = cl.epoch;
    va.tf = cl.tf;
    va.work = cl.work;
    va.s_tf = cl.s_tf;
    va.s_work = cl.s_work;
  }

  // the off-cell fixup of the batch captured as cl on buffer set c (grids: its frames' canvases)
  void fixup_args(const c3h_ctx* c, const c3h::C3Launch& cl, const uint32_t* const* grids, int f0, int nb,
                  c3h::PointFixup& fx) const {
    fx.nf = nb;
    for (int j = 0; j < nb; ++j) fx.grid[j] = grids[j];
    fx.moved = c->pb_moved.p;
    fx.xcnt = c->pb_xcnt.p;
    fx.info = ctx->pb_info.p + f0;
    for (int a = 0; a < 3; ++a) {
      fx.C[a] = canvas[a];
      fx.thr[a] = cl.thr[a];
    }
    fx.axmap = cl.axmap;
    fx.segs = cl.segs;
    fx.ns0 = cl.nseg[0];
    fx.ns1 = cl.nseg[1];
    fx.seg_stride = cl.seg_stride;
    fx.sbx = cl.sbx;
    fx.sby = cl.sby;
    fx.variant = cl.variant;
    fx.lut = cl.lut;
    fx.feat = cl.feat;
    fx.exist = cl.exist;
    fx.rows = cl.rows;
    fx.tf = cl.tf;
    fx.s_feat = cl.s_feat;
    fx.s_h = cl.s_h;
    fx.s_tf = cl.s_tf;
    fx.epoch = cl.epoch;
    for (int a = 0; a < 3; ++a) fx.lmax[a] = cl.lmax[a];
  }

  // Reads the frames' records back into fi and decides which frames the single-frame path
  // runs again (redo).  exact_ran: per frame, its batch ran the exact pass + fixup.
  int read_records(bool canvas_multi, const std::vector<char>& exact_ran, std::vector<c3h_frame_info>& fi,
                   std::vector<char>& redo) {
    // the records come back through pinned memory: one asynchronous copy and one stream
    // synchronisation (a pageable copy blocks, then the stream is synchronised again; ~20 us
    // of a 64-frame call's ~0.75 ms)
    if (ctx->h_recs_n < (size_t)src.nframes) {
      if (ctx->h_recs) HIPCHK(hipHostFree(ctx->h_recs));
      ctx->h_recs = nullptr;
      ctx->h_recs_n = 0;
      void* hp = nullptr;
      HIPCHK(hipHostMalloc(&hp, (size_t)src.nframes * sizeof(c3h::VoxFrameRec)));
      ctx->h_recs = static_cast<c3h::VoxFrameRec*>(hp);
      ctx->h_recs_n = (size_t)src.nframes;
    }
    const c3h::VoxFrameRec* recs = ctx->h_recs;
    HIPCHK(hipMemcpyAsync(ctx->h_recs, ctx->pb_info.p, (size_t)src.nframes * sizeof(c3h::VoxFrameRec),
                          hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < src.nframes; ++i) {
      const c3h::VoxFrameRec& r = recs[i];
      c3h_frame_info& o = fi[i];
      bool one = true;
      for (int a = 0; a < 3; ++a) {
        o.min_b[a] = r.min_b[a];
        o.div_b[a] = r.max_b[a] - r.min_b[a] + 1;
        o.subdiv_b[a] = p->subdiv > 0 ? r.sb[a] : 0;  // getSubdivNum without subdivisions: 0
        one = one && r.sb[a] == 1;
      }
      o.n_valid = r.n_valid;
      o.n_occ = r.n_occ;
      o.n_moved = (int32_t)r.moved;
      o.status = 0;
      const bool hist1_mismatch = p->subdiv > 0 && canvas_multi && one;
      const bool empty_sub = p->subdiv > 0 && (r.sb[0] == 0 || r.sb[1] == 0 || r.sb[2] == 0);
      redo[i] = (r.err || (r.flagged && !exact_ran[i]) || r.n_valid == 0 || hist1_mismatch || empty_sub) ? 1 : 0;
    }
    return C3H_OK;
  }
};

// Points-in batches: the scatter stamps the tick's tiles (a canvas that does not match the
// grid: the tick streams the canvases), and flagged voxels are summed exactly and off-cell
// voxels fixed up in the batch.  The body of both points-in entry points.
int run_point_source(c3h_ctx* ctx, const PointSrc& src, float leaf, float z_limit, const int32_t canvas[3],
                     const c3h_extract_params* p, const int32_t range[3], int32_t exist_threshold, int32_t rotate,
                     c3h_det* d_out, c3h_frame_info* info) {
  const int32_t nframes = src.nframes;
  const std::string& who = src.who;
  if (p->variant != 981 && p->variant != 117) return fail(ctx, C3H_ERR_ARG, who + ": variant");
  if (p->color_mode < C3H_COLOR_C3_FLOAT || p->color_mode > C3H_COLOR_CHLAC)
    return fail(ctx, C3H_ERR_ARG, who + ": color_mode");
  if (int rc = overlap_rank_check(ctx, who.c_str())) return rc;
  int64_t cvox = 1;
  for (int a = 0; a < 3; ++a) {
    if (canvas[a] < 1) return fail(ctx, C3H_ERR_ARG, who + ": canvas dims must be >= 1");
    cvox *= canvas[a];
  }
  if (cvox > 2147483647LL) return fail(ctx, C3H_ERR_RANGE, who + ": canvas beyond int32 voxel indices");
  HIPCHK(hipSetDevice(ctx->device));
  if (int rc = pipe_flush(ctx)) return rc;  // an open frame stream completes first
  if (nframes == 0) return 0;
  const size_t per_frame = (size_t)std::max(ctx->M, 1) * ctx->rank;
  std::vector<c3h_frame_info> fi((size_t)nframes);
  std::vector<char> redo((size_t)nframes, 1);
  int modes[6];  // the modes the search schedules (search.cpp:384-417): the single-frame path's count
  int nm = mode_schedule(range[0], range[1], range[2], rotate, modes);
  const int nm_sched = nm;
  std::vector<char> exact_ran((size_t)nframes, 0);  // per frame: its batch ran the exact pass + fixup
  // canvas subdivisions: a frame with one subdivision where the canvas has several takes the
  // single-frame path (computeC3HLAC's hist_num == 1 rule puts every voxel in histogram 0)
  bool canvas_multi = false;
  if (p->subdiv > 0) {
    const float inv_s = 1.0 / p->subdiv;
    int64_t hn = 1;
    for (int a = 0; a < 3; ++a) hn *= canvas[a] > p->offset[a] ? (int64_t)ceilf((canvas[a] - p->offset[a]) * inv_s) : 0;
    canvas_multi = hn > 1;
  }
  const bool batched = pipelinable(ctx) && p->subdiv >= 0 && p->thr[0] >= 0 && p->thr[1] >= 0 && p->thr[2] >= 0;
  if (batched) {
    const int B = std::max(1, std::min(ctx->nbatch, c3h::kMaxBatch));
    const int nchunks = (nframes + B - 1) / B;
    int rc = ensure_lanes(ctx, kPipeDepth - 1);
    if (rc != C3H_OK) return rc;
    const int32_t zero[3] = {0, 0, 0};
    const c3h_ctx::PipeKey k = pipe_key(ctx, canvas, zero, leaf, p, range, exist_threshold, rotate, B);
    PointCall pc{ctx, src, leaf, z_limit, canvas, p, cvox, B, c3h::vb_chunk()};
    if (int e = pc.shared_setup()) return e;
    // overlap pays where the tick is light: 512 x 128^3 frames 51k -> 74k frames/s.  While
    // the tick streamed the canvases, 256^3 lost with it (33k -> 30k: the 67 MB grid stream
    // and the voxeliser's atomics slowed each other down, profiles/r3/points_overlap/); with
    // the scatter's stamps (no canvas stream) it gains there too: 41k -> 45k frames/s
    // (profiles/r3/point_stamp/).  Canvases up to 2^25 voxels (256^3 and a little beyond)
#ifndef C3H_POINT_OVERLAP_VOX
#define C3H_POINT_OVERLAP_VOX (1 << 25)
#endif
    const bool overlap = cvox <= (int64_t)C3H_POINT_OVERLAP_VOX;
    const hipStream_t vs = overlap ? ctx->pb_vstream : ctx->stream;
    // every exit (errors included) leaves the voxeliser stream idle: the next call may
    // reallocate the buffers its work reads
    struct VsIdle {
      hipStream_t s;
      ~VsIdle() { (void)hipStreamSynchronize(s); }
    } vs_idle{vs};
    // the voxeliser stream starts after everything enqueued so far (the memsets above)
    HIPCHK(hipEventRecord(ctx->pb_vox_ev, ctx->stream));
    HIPCHK(hipStreamWaitEvent(vs, ctx->pb_vox_ev, 0));
    PipeScope scope(ctx);
    for (int ch = 0; ch < nchunks && rc >= 0; ++ch) {
      const int f0 = ch * B, nb = std::min(B, nframes - f0);
      c3h_ctx* c = pipe_set(ctx, ctx->pipe_seq);
      // the batch's voxeliser arguments (a buffer set that has to grow is reallocated in there,
      // both streams idle; host frames' staging copies go on the voxeliser stream)
      c3h::VoxBatchArgs va{};
      if (int e = pc.vox_args(c, f0, nb, vs, va)) return e;
      const uint32_t* grids[c3h::kMaxBatch];
      c3h_det* outs[c3h::kMaxBatch];
      for (int j = 0; j < nb; ++j) {
        grids[j] = c->pb_grid.p + (size_t)j * cvox;
        outs[j] = d_out + (size_t)(f0 + j) * per_frame;
      }
      // the accumulate needs nothing of the batch's C3 launch, so it starts before the
      // launch is captured (the capture's host work, ~10 us, then runs beside it: a one-batch
      // call starts sooner).  The set's grids and gate limits were last read by the tick
      // pushed two batches ago (tile role: one tick after the batch's own, gate role: two),
      // so this batch's voxels overlap the previous batch's tick
      if (ch >= 2) HIPCHK(hipStreamWaitEvent(vs, ctx->pb_tick_ev[(ch - 2) & 3], 0));
      {
        Timed t(ctx, 0, nb, vs);
        HIPCHK(c3h::launch_vox_batch_accum(va, vs));
      }
      // until the chain below has run, the accumulators hold this batch's sums: an exit in
      // between has the next call re-zero them
      struct PbAccGuard {
        c3h_ctx* c;
        bool armed;
        ~PbAccGuard() {
          if (armed) c->pb_acc_vox = 0;
        }
      } pb_acc_guard{ctx, true};
      // the batch's launches are captured next: the scatter sets its tile stamps and work
      // lists (the occupancy stream's job), so its first tick carries no occupancy role and
      // no canvas is streamed (128^3: 8.4 MB, 256^3: 67 MB per frame)
      c3h_ctx::PipeBatch fresh{};
      const int h2d0 = c->cap_h2d;
      rc = pipe_prepare(ctx, grids, outs, nb, k, c->pb_lim.p, &fresh);
      if (rc == 0) rc = fail(ctx, C3H_ERR_STATE, who + ": the canvas does not fit the pipeline");
      if (rc < 0) break;
      const c3h::C3Launch& cl = fresh.l;
      pc.launch_args(cl, va);
      // the exact pass + off-cell fixup: the tick's direct mode (a row list, one tile per
      // subdivision) on the canvas itself; otherwise flagged frames take the single-frame path
      const bool exact = cl.rows && cl.axmap && cl.gx == canvas[0] && cl.gy == canvas[1] &&
                         cl.gz == canvas[2] && c3h::point_fixup_fits(cl.lmax);
      if (exact) {
        va.flags = c->pb_flags.p;
        va.bucket = c->pb_bucket.p;
        va.moved = c->pb_moved.p;
        va.xcnt = c->pb_xcnt.p;
        pc.fixup_args(c, cl, grids, f0, nb, fresh.fx);
        fresh.fix = true;
      }
      if (exact) std::fill(exact_ran.begin() + f0, exact_ran.begin() + f0 + nb, (char)1);
      // tables / stamp resets the capture enqueued precede the stamps (first batches only)
      if (va.stamp && vs != ctx->stream && c->cap_h2d != h2d0) {
        HIPCHK(hipEventRecord(ctx->pb_vox_ev, ctx->stream));
        HIPCHK(hipStreamWaitEvent(vs, ctx->pb_vox_ev, 0));
      }
      {
        Timed t(ctx, 0, 0, vs);  // (the frames are counted with the accumulate)
        HIPCHK(c3h::launch_vox_batch_post(va, vs));
      }
      pb_acc_guard.armed = false;  // the scatter returns every touched accumulator to zero
      HIPCHK(hipEventRecord(ctx->pb_vox_ev, vs));
      c->pb_prev_nf = nb;
      c->pb_prev_total = va.total;
      c->pb_prev_blk0.assign(va.blk0, va.blk0 + nb + 1);
      fresh.stamped = va.stamp != 0;
      // A stamped batch has no role in its own first tick (that tick runs the tile role of
      // the batch before it, compress + gate and scoring of older ones), so the tick goes
      // ahead of this batch's voxeliser and only the next tick waits for it (round 6: the
      // batch's tile role then runs beside the next voxeliser instead of after it, one
      // tick less per call after the last voxeliser).  An unstamped batch's first tick
      // streams its canvases: it waits.
      if (!fresh.stamped) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->pb_vox_ev, 0));
      if (fresh.nosearch)  // no search: the frames' lists are the fresh setRank state
        HIPCHK(hipMemsetAsync(d_out + (size_t)f0 * per_frame, 0, (size_t)nb * per_frame * sizeof(c3h_det), ctx->stream));
      rc = pipe_commit(ctx, fresh, k, rc);
      if (rc > 0) nm = fresh.nosearch ? nm_sched : rc;  // (no search: as the single-frame path)
      if (rc >= 0) HIPCHK(hipEventRecord(ctx->pb_tick_ev[ch & 3], ctx->stream));
      if (fresh.stamped) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->pb_vox_ev, 0));
    }
    if (rc < 0) ctx->pipe.clear();
    else rc = pipe_drain(ctx);
    if (rc < 0) return rc;
    if (int e = pc.read_records(canvas_multi, exact_ran, fi, redo)) return e;
  }
  for (int i = 0; i < nframes; ++i) {
    if (!redo[i]) continue;
    int rc = point_src_single(ctx, src, i, leaf, z_limit, p, range, exist_threshold, rotate,
                              d_out + (size_t)i * per_frame, &fi[i]);
    if (rc == C3H_ERR_HIP || rc == C3H_ERR_NOMEM) return rc;  // device trouble ends the call
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (info) memcpy(info, fi.data(), fi.size() * sizeof(c3h_frame_info));
  return nm;
}

}  // namespace

extern "C" {

int c3h_run_point_frames(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device,
                         float leaf, float z_limit, const int32_t canvas[3], const c3h_extract_params* p,
                         const int32_t range[3], int32_t exist_threshold, int32_t rotate, c3h_det* d_out,
                         c3h_frame_info* info) {
  if (!ctx || !pts || !n || nframes < 0 || !canvas || !p || !range || !d_out || !(leaf > 0)) return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, "c3h_run_point_frames: no axes (call c3h_search_setup)");
  for (int i = 0; i < nframes; ++i)
    if (n[i] < 0 || (n[i] > 0 && !pts[i]) || n[i] >= ((int64_t)1 << 24))
      return fail(ctx, C3H_ERR_ARG, "c3h_run_point_frames: frame point counts must be in [0, 16,777,215]");
  PointSrc src;
  src.who = "c3h_run_point_frames";
  src.base = reinterpret_cast<const void* const*>(pts);
  src.n = n;
  src.nframes = nframes;
  src.on_device = on_device;
  return run_point_source(ctx, src, leaf, z_limit, canvas, p, range, exist_threshold, rotate, d_out, info);
}

int c3h_run_pointcloud2_frames(c3h_ctx* ctx, const void* const* data, const uint32_t* height, const uint32_t* width,
                               const uint32_t* row_step, int32_t nframes, const c3h_pc2_layout* layout, int on_device,
                               float leaf, float z_limit, const int32_t canvas[3], const c3h_extract_params* p,
                               const int32_t range[3], int32_t exist_threshold, int32_t rotate, c3h_det* d_out,
                               c3h_frame_info* info) {
  if (!ctx || nframes < 0 || (nframes > 0 && (!data || !height || !width || !row_step)) || !layout || !canvas || !p ||
      !range || !d_out || !(leaf > 0))
    return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, "c3h_run_pointcloud2_frames: no axes (call c3h_search_setup)");
  std::vector<int64_t> n((size_t)nframes);
  uint64_t base_or = 0;
  uint32_t row_step_or = 0;
  for (int i = 0; i < nframes; ++i) {
    int rc = pc2_check(ctx, height[i], width[i], layout->point_step, row_step[i], layout->offsets);
    if (rc != C3H_OK) return rc;
    n[i] = (int64_t)height[i] * width[i];
    if (n[i] > 0 && !data[i]) return fail(ctx, C3H_ERR_ARG, "pointcloud2: no data");
    if (n[i] >= (int64_t)1 << 24)
      return fail(ctx, C3H_ERR_RANGE, "c3h_run_pointcloud2_frames: at most 16,777,215 points per message");
    if (n[i] == 0) continue;
    // host messages are staged at 16-byte aligned addresses
    if (on_device) base_or |= (uint64_t)(uintptr_t)data[i];
    if (!c3h::pc2_flat(height[i], width[i], layout->point_step, row_step[i])) row_step_or |= row_step[i];
  }
  PointSrc src;
  src.who = "c3h_run_pointcloud2_frames";
  src.base = data;
  src.n = n.data();
  src.nframes = nframes;
  src.on_device = on_device;
  src.layout = layout;
  src.height = height;
  src.width = width;
  src.row_step = row_step;
  src.plan = c3h::pc2_plan(layout->point_step, layout->offsets, layout->is_bigendian, base_or, row_step_or);
  return run_point_source(ctx, src, leaf, z_limit, canvas, p, range, exist_threshold, rotate, d_out, info);
}

}  // extern "C"
