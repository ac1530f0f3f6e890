// capi_vosch.hip -- point clouds in, VOSCH / GRSD rows out, for a batch of frames
// (c3h_extract_vosch_frames, c3h_run_vosch_point_frames and their getters).
//
// Per frame, in turn, the single-frame code computes what only it can: the voxel grid
// (c3h_voxelize, which synchronises the host once per frame), the exact centroids, the leaf
// layout and, at dim 137, the C3-HLAC-117 rows (extract_frames), whose columns go straight into
// the frame's output rows.  What a frame leaves for the batch is small: its geometry on the
// host, its centroids in leaf order and their voxel keys in batch slots.  Everything else --
// search grids, normals, RSD, GRSD transitions, columns 0 .. 19 -- runs once per batch
// (vosch_front.hip) over a device table of per-frame records.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_host.h"

using c3h::fail;

namespace {

struct FrontFrame {
  c3h::VfGrid g, g2;
  int32_t sb[3];
  int64_t H, nc, n;
  float inv_s;
  c3h_grid_info gi;
  const float4* pts;
};

// One frame through the single-frame head.  Returns its status (0, or the error the
// single-frame route -- c3h_voxelize, c3h_compute_normals, c3h_extract_vosch / _grsd -- gives);
// on success the frame's centroids, voxel keys and C3 columns are enqueued.
int front_head(c3h_ctx* ctx, const float* pts, int64_t n, int on_device, float leaf, float z_limit,
               const c3h_vosch_params* p, int dim, int64_t row_cap, float max_dist, bool wide, int64_t p0, int64_t v0,
               float* rows, FrontFrame* fr) {
  int rc = c3h_voxelize(ctx, pts, n, on_device, leaf, z_limit, &fr->gi);
  if (rc != C3H_OK) return rc;
  if (!ctx->have_grid || !ctx->table_valid)
    return fail(ctx, C3H_ERR_STATE, "compute_normals: needs the points of a c3h_voxelize");
  if (c3h::vf_nbr_grid(fr->gi.min_b, fr->gi.max_b, ctx->info.leaf, p->normals_radius, &fr->g) != c3h::kVfOk)
    return fail(ctx, C3H_ERR_RANGE, "normals: more than 2^27 search cells");
  fr->g2 = fr->g;
  fr->H = c3h::vf_subdivisions(fr->gi.div_b, p->grsd.subdiv, p->grsd.offset, fr->sb, &fr->inv_s);
  if (fr->H > row_cap) return fail(ctx, C3H_ERR_RANGE, "vosch frames: a frame has more rows than row_cap");
  rc = c3h::grsd_frame_head(ctx, &p->grsd, fr->sb, &fr->H, &fr->inv_s);
  if (rc != C3H_OK) return rc;
  if (fr->H > 0 && wide && c3h::vf_nbr_grid(fr->gi.min_b, fr->gi.max_b, ctx->info.leaf, max_dist, &fr->g2) != c3h::kVfOk)
    return fail(ctx, C3H_ERR_RANGE, "normals: more than 2^27 search cells");
  fr->n = n;
  fr->nc = fr->H > 0 ? fr->gi.n_occ : 0;
  fr->pts = reinterpret_cast<const float4*>(pts);
  if (!on_device) {  // c3h_voxelize staged the host points in ctx->pts: the next frame overwrites them
    HIPCHK(hipMemcpyAsync(ctx->vf_pts.p + p0, ctx->pts.p, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
    fr->pts = ctx->vf_pts.p + p0;
  }
  if (fr->nc > 0) {
    const int64_t nvox = (int64_t)fr->gi.div_b[0] * fr->gi.div_b[1] * fr->gi.div_b[2];
    HIPCHK(hipMemcpyAsync(ctx->vf_cent.p + v0, ctx->dsamp.p, (size_t)fr->nc * 16, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(c3h::launch_vf_vox_keys(ctx->tmp_i32.p, nvox, fr->nc, ctx->vf_vkeys.p + v0, ctx->stream));
  }
  if (dim == 137) {  // the C3 part of extractVOSCH, as c3h_extract_vosch runs it
    c3h_extract_params e{};
    e.variant = 117;
    for (int a = 0; a < 3; ++a) {
      e.thr[a] = p->thr[a];
      e.offset[a] = p->grsd.offset[a];
    }
    e.subdiv = p->grsd.subdiv;
    e.color_mode = p->color_mode;
    const uint32_t* g = ctx->grid_ptr;
    int32_t sb2[3];
    int64_t H2 = 0;
    rc = c3h::extract_frames(ctx, &g, 1, &e, sb2, &H2);
    if (rc != C3H_OK) return rc;
    if (H2 != fr->H) return fail(ctx, C3H_ERR_STATE, "extract_vosch: GRSD / C3 subdivisions differ");
    HIPCHK(c3h::launch_vf_c3_cols(ctx->feat.p, ctx->exist.p, fr->H, rows, ctx->stream));
  }
  return C3H_OK;
}

// The front end of both entry points: frame i's rows at d_rows + i * row_cap * dim, info[i]
// filled (info != nullptr).  Returns C3H_OK or the error that stopped the call.
int vosch_front(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device, float leaf,
                float z_limit, const c3h_vosch_params* p, int32_t dim, int64_t row_cap, float* d_rows,
                c3h_frame_info* info) {
  HIPCHK(hipSetDevice(ctx->device));
  const int B = std::max(1, std::min(ctx->nbatch, c3h::kVfMaxFrames));
  ctx->vf_nframes = 0;
  ctx->vf_n.assign(n, n + nframes);
  ctx->vf_status.assign((size_t)nframes, 0);
  ctx->vf_ppre.assign((size_t)nframes + 1, 0);
  ctx->vf_vpre.assign((size_t)nframes + 1, 0);
  // RSD radius: max(rsd_radius_search, voxel_size / 2 * sqrt(3)) (grsd_colorCHLAC_tools.hpp:172); beyond
  // 4 x the normals' cell the RSD gets a grid of its own radius (grsd_frames)
  const float max_dist = (float)std::max((double)p->grsd.rsd_radius, (double)leaf / 2 * std::sqrt(3.0));
  const bool wide = max_dist > 4 * p->normals_radius;
  const float vp0[3] = {p->viewpoint[0], p->viewpoint[1], p->viewpoint[2]};
  ctx->vf_htab.resize(1);  // lives with the context: its upload is asynchronous
  c3h::VfTable* const ht = ctx->vf_htab.data();
  std::vector<FrontFrame> ff((size_t)B);
  for (int b0 = 0; b0 < nframes; b0 += B) {
    const int nb = std::min(B, nframes - b0);
    int64_t upper = 0;
    for (int j = 0; j < nb; ++j) upper += std::max<int64_t>(n[b0 + j], 0);
    if (upper > c3h::kVfMaxPoints) return fail(ctx, C3H_ERR_RANGE, "vosch frames: a batch holds 2^32 points or more");
    // the previous batch's table upload and launches read *ht and the buffers that may grow now
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!on_device) ENSURE(ctx->vf_pts, upper);
    ENSURE(ctx->vf_cent, upper);
    ENSURE(ctx->vf_vkeys, upper);
    memset(ht, 0, sizeof(c3h::VfTable));
    ht->nf = nb;
    int64_t max_cells = 1;
    for (int j = 0; j < nb; ++j) {
      const int i = b0 + j;
      FrontFrame& fr = ff[(size_t)j];
      fr = FrontFrame{};
      c3h_frame_info& fi = info[i];
      memset(&fi, 0, sizeof(fi));
      float* rows = d_rows + (size_t)i * row_cap * dim;
      const int st = front_head(ctx, pts[i], n[i], on_device, leaf, z_limit, p, dim, row_cap, max_dist, wide, ht->ppre[j],
                                ht->vpre[j], rows, &fr);
      fi.status = st;
      ctx->vf_status[(size_t)i] = st;
      if (st < 0) fr = FrontFrame{};  // no points, cells, centroids or rows in the batch
      else {
        for (int a = 0; a < 3; ++a) {
          fi.div_b[a] = fr.gi.div_b[a];
          fi.min_b[a] = fr.gi.min_b[a];
          fi.subdiv_b[a] = fr.sb[a];
        }
        fi.n_valid = fr.gi.n_valid;
        fi.n_occ = fr.gi.n_occ;
        fi.n_moved = fr.H > 0 ? (int32_t)ctx->n_offcell : 0;
        max_cells = std::max(max_cells, std::max(fr.g.ncell, fr.g2.ncell));
      }
      ht->ppre[j + 1] = ht->ppre[j] + fr.n;
      ht->cpre[j + 1] = ht->cpre[j] + (st < 0 ? 0 : fr.g.ncell);
      ht->c2pre[j + 1] = ht->c2pre[j] + (st < 0 ? 0 : fr.g2.ncell);
      ht->vpre[j + 1] = ht->vpre[j] + fr.nc;
      ht->hpre[j + 1] = ht->hpre[j] + fr.H;
      if (nframes <= B) {
        ctx->vf_ppre[(size_t)i + 1] = ht->ppre[j + 1];
        ctx->vf_vpre[(size_t)i + 1] = ht->vpre[j + 1];
      }
    }
    const int64_t ptot = ht->ppre[nb], ctot = ht->cpre[nb], c2tot = ht->c2pre[nb], vtot = ht->vpre[nb], htot = ht->hpre[nb];
    if (ptot == 0) continue;
    c3h::VfKey key{};
    if (c3h::vf_key(max_cells, nb, ptot, &key) != c3h::kVfOk)
      return fail(ctx, C3H_ERR_RANGE, "vosch frames: the batch does not fit the composite sort key");
    const size_t kw = key.wide ? 1 : 2;  // keys per 64-bit word
    ENSURE(ctx->vf_keys, ((size_t)ptot + kw - 1) / kw);
    ENSURE(ctx->vf_keys2, ((size_t)ptot + kw - 1) / kw);
    ENSURE(ctx->vf_idx, ptot);
    ENSURE(ctx->vf_idx2, ptot);
    ENSURE(ctx->vf_cstart, std::max(ctot, c2tot));
    ENSURE(ctx->vf_cend, std::max(ctot, c2tot));
    ENSURE(ctx->vf_normals, ptot);
    ENSURE(ctx->vf_types, vtot);
    ENSURE(ctx->vf_radii, vtot);
    ENSURE(ctx->vf_trans, htot * 36);
    ENSURE(ctx->vf_tab, 1);
    ENSURE(ctx->vf_dense, c3h::vf_dense_cap(ptot) + 1);
    for (int j = 0; j < nb; ++j) {
      const FrontFrame& fr = ff[(size_t)j];
      c3h::VfFrame& t = ht->fr[j];
      for (int which = 0; which < 2; ++which) {
        const c3h::VfGrid& vg = which ? fr.g2 : fr.g;
        c3h::NbrGrid& g = which ? t.g2 : t.g;
        g.pts = fr.pts;
        g.n = fr.n;
        g.z_limit = z_limit;
        g.cell = vg.cell;
        g.inv_cell = vg.inv_cell;
        for (int a = 0; a < 3; ++a) {
          g.origin[a] = vg.origin[a];
          g.dim[a] = vg.dim[a];
        }
        g.sorted = ctx->vf_idx2.p + ht->ppre[j];
        g.cstart = ctx->vf_cstart.p + (which ? ht->c2pre[j] : ht->cpre[j]);
        g.cend = ctx->vf_cend.p + (which ? ht->c2pre[j] : ht->cpre[j]);
      }
      c3h::GrsdArgs& ga = t.ga;
      ga.cent = ctx->vf_cent.p + ht->vpre[j];
      ga.nc = fr.nc;
      ga.layout = nullptr;
      ga.types = ctx->vf_types.p + ht->vpre[j];
      ga.trans = ctx->vf_trans.p + ht->hpre[j] * 36;
      for (int a = 0; a < 3; ++a) {
        ga.div_b[a] = fr.gi.div_b[a];
        ga.min_b[a] = fr.gi.min_b[a];
        ga.off[a] = p->grsd.subdiv > 0 ? p->grsd.offset[a] : 0;
        ga.sb[a] = fr.sb[a];
      }
      ga.leaf = fr.gi.leaf;
      ga.inv_leaf = 1.0f / fr.gi.leaf;
      ga.inv_s = fr.inv_s;
      ga.hist1 = fr.H == 1 ? 1 : 0;
      t.vkeys = ctx->vf_vkeys.p + ht->vpre[j];
      t.rows = d_rows + (size_t)(b0 + j) * row_cap * dim;
    }
    HIPCHK(hipMemcpyAsync(ctx->vf_tab.p, ht, sizeof(c3h::VfTable), hipMemcpyHostToDevice, ctx->stream));
    size_t tb = 0;
    HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 0, key, ptot, ctot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                             ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, nullptr, &tb, ctx->stream));
    ENSURE(ctx->vf_tmp, std::max<size_t>(tb, 1));
    tb = ctx->vf_tmp.n;
    HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 0, key, ptot, ctot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                             ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, ctx->vf_tmp.p, &tb, ctx->stream));
    const int reach = c3h::vf_reach(p->normals_radius, 1.0f / p->normals_radius);
    if (reach > c3h::kVfMaxReach) return fail(ctx, C3H_ERR_STATE, "vosch frames: internal: normals reach");
    HIPCHK(c3h::launch_vf_normals(ctx->vf_tab.p, key, ptot, ctot, ctx->vf_keys2.p, ctx->vf_dense.p, p->normals_radius, reach, vp0,
                                  ctx->vf_normals.p, ctx->stream));
    if (vtot > 0) {
      const float rsd_cell = wide ? max_dist : p->normals_radius;
      if (wide)  // (the normals are done with the first grid: its buffers take the second)
        HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 1, key, ptot, c2tot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                                 ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, ctx->vf_tmp.p, &tb, ctx->stream));
      HIPCHK(c3h::launch_vf_rsd(ctx->vf_tab.p, vtot, ctx->vf_normals.p, max_dist, c3h::vf_reach(max_dist, 1.0f / rsd_cell),
                                ctx->vf_radii.p, ctx->vf_types.p, ctx->stream));
    }
    if (htot > 0) {
      HIPCHK(hipMemsetAsync(ctx->vf_trans.p, 0, (size_t)htot * 36 * 4, ctx->stream));
      HIPCHK(c3h::launch_vf_grsd(ctx->vf_tab.p, vtot, ctx->stream));
      // NORMALIZE_GRSD = 20 / 26 (grsd_colorCHLAC_tools.h:32) when is_normalize
      HIPCHK(c3h::launch_vf_rows(ctx->vf_tab.p, htot, ctx->vf_trans.p, p->grsd.normalize ? (float)(20.0 / 26) : 1.0f, dim,
                                 ctx->stream));
    }
  }
  ctx->vf_nframes = nframes <= B ? nframes : -1;
  return C3H_OK;
}

int front_args(c3h_ctx* ctx, const char* who, const float* const* pts, const int64_t* n, int32_t nframes, float leaf,
               const c3h_vosch_params* p, int32_t dim) {
  if (!ctx || !p || nframes < 0 || (nframes > 0 && (!pts || !n))) return C3H_ERR_ARG;
  if (dim != 137 && dim != 20) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": dim must be 137 (VOSCH) or 20 (GRSD)");
  if (!(leaf > 0) || !(p->normals_radius > 0)) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": leaf and normals_radius must be > 0");
  return C3H_OK;
}

int frame_check(c3h_ctx* ctx, const char* who, int32_t frame) {
  if (ctx->vf_nframes < 0) return fail(ctx, C3H_ERR_STATE, std::string(who) + ": the last call had more than one batch");
  if (ctx->vf_nframes == 0) return fail(ctx, C3H_ERR_STATE, std::string(who) + ": no c3h_extract_vosch_frames call");
  if (frame < 0 || frame >= ctx->vf_nframes) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": no such frame");
  if (ctx->vf_status[(size_t)frame] < 0) return fail(ctx, C3H_ERR_STATE, std::string(who) + ": the frame failed");
  return C3H_OK;
}

}  // namespace

extern "C" {

int c3h_extract_vosch_frames(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device,
                             float leaf, float z_limit, const c3h_vosch_params* p, int32_t dim, int64_t row_cap,
                             float* d_rows, c3h_frame_info* info) {
  int rc = front_args(ctx, "c3h_extract_vosch_frames", pts, n, nframes, leaf, p, dim);
  if (rc != C3H_OK) return rc;
  if (row_cap < 0 || (nframes > 0 && row_cap > 0 && !d_rows))
    return fail(ctx, C3H_ERR_ARG, "c3h_extract_vosch_frames: row_cap / d_rows");
  QUIESCE(ctx);
  std::vector<c3h_frame_info> own;
  if (!info) {
    own.resize((size_t)std::max(nframes, 1));
    info = own.data();
  }
  return vosch_front(ctx, pts, n, nframes, on_device, leaf, z_limit, p, dim, row_cap, d_rows, info);
}

int c3h_run_vosch_point_frames(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device,
                               float leaf, float z_limit, const c3h_vosch_params* p, int32_t dim,
                               const int32_t canvas_b[3], const int32_t range[3], int32_t exist_threshold,
                               int32_t rotate, c3h_det* d_out, c3h_frame_info* info) {
  const char* who = "c3h_run_vosch_point_frames";
  int rc = front_args(ctx, who, pts, n, nframes, leaf, p, dim);
  if (rc != C3H_OK) return rc;
  if (!canvas_b || !range || !d_out) return C3H_ERR_ARG;
  if (!ctx->have_setup) return fail(ctx, C3H_ERR_STATE, std::string(who) + ": no axes (call c3h_search_setup)");
  if (dim != ctx->F) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": dim differs from the F of c3h_search_setup");
  if (range[0] < 1 || range[1] < 1 || range[2] < 1) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": ranges must be >= 1");
  int64_t cap = 1;
  for (int a = 0; a < 3; ++a) {
    if (canvas_b[a] < 0) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": canvas_b");
    cap *= canvas_b[a];
  }
  if (cap > INT32_MAX) return fail(ctx, C3H_ERR_RANGE, std::string(who) + ": canvas beyond int32 row indices");
  QUIESCE(ctx);
  std::vector<c3h_frame_info> own;
  if (!info) {
    own.resize((size_t)std::max(nframes, 1));
    info = own.data();
  }
  ENSURE(ctx->vf_rows, (size_t)std::max(nframes, 1) * std::max<int64_t>(cap, 1) * dim);
  rc = vosch_front(ctx, pts, n, nframes, on_device, leaf, z_limit, p, dim, cap, ctx->vf_rows.p, info);
  if (rc != C3H_OK) return rc;
  std::vector<const float*> feats((size_t)std::max(nframes, 1), nullptr);
  std::vector<int32_t> sbs((size_t)std::max(nframes, 1) * 3, 0);
  for (int i = 0; i < nframes; ++i) {
    c3h_frame_info& fi = info[i];
    if (fi.status >= 0 && (fi.subdiv_b[0] > canvas_b[0] || fi.subdiv_b[1] > canvas_b[1] || fi.subdiv_b[2] > canvas_b[2])) {
      fi.status = C3H_ERR_RANGE;  // (its rows fit the product, its counts do not fit the canvas)
      ctx->vf_status[(size_t)i] = C3H_ERR_RANGE;
    }
    feats[(size_t)i] = ctx->vf_rows.p + (size_t)i * cap * dim;
    if (fi.status >= 0)
      for (int a = 0; a < 3; ++a) sbs[(size_t)i * 3 + a] = fi.subdiv_b[a];
  }
  // the body of c3h_run_feature_frames: failed frames go in with counts (0, 0, 0) and yield the setRank state
  return c3h_run_feature_frames(ctx, feats.data(), nullptr, nframes, sbs.data(), canvas_b, dim,
                                dim == 137 ? C3H_EXIST_VOSCH : C3H_EXIST_GRSD, range, exist_threshold, rotate, d_out);
}

int c3h_get_frame_normals(c3h_ctx* ctx, int32_t frame, float* out, int on_device) {
  if (!ctx || !out) return C3H_ERR_ARG;
  QUIESCE(ctx);
  int rc = frame_check(ctx, "c3h_get_frame_normals", frame);
  if (rc != C3H_OK) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n = ctx->vf_n[(size_t)frame];
  if (n > 0)
    HIPCHK(hipMemcpyAsync(out, ctx->vf_normals.p + ctx->vf_ppre[(size_t)frame], (size_t)n * 16,
                          on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return C3H_OK;
}

int c3h_get_frame_rsd(c3h_ctx* ctx, int32_t frame, float* radii, int32_t* types, int on_device) {
  if (!ctx) return C3H_ERR_ARG;
  QUIESCE(ctx);
  int rc = frame_check(ctx, "c3h_get_frame_rsd", frame);
  if (rc != C3H_OK) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t v0 = ctx->vf_vpre[(size_t)frame], nc = ctx->vf_vpre[(size_t)frame + 1] - v0;
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (radii && nc) HIPCHK(hipMemcpyAsync(radii, ctx->vf_radii.p + v0, (size_t)nc * 8, k, ctx->stream));
  if (types && nc) HIPCHK(hipMemcpyAsync(types, ctx->vf_types.p + v0, (size_t)nc * 4, k, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return (int)std::min<int64_t>(nc, INT32_MAX);
}

}  // extern "C"
