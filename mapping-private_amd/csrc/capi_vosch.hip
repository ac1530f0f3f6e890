// capi_vosch.hip -- normals, RSD, GRSD and VOSCH rows of point clouds: the host side of the
// front (vosch_front.hip) for one frame (c3h_compute_normals, c3h_extract_grsd,
// c3h_extract_vosch and their getters) and for a batch of frames (c3h_extract_vosch_frames,
// c3h_run_vosch_point_frames and theirs), and c3h_extract_c3_frames: the batched voxel head and the
// sparse C3-HLAC pass without the front (c3_rows_front), with c3h_extract_c3_frames_packed and
// c3h_pca_add_c3_frames on its packed mode (only the rows that hold a voxel, one after another).
//
// The head of a batch gives the front what only a voxeliser can: every frame's voxel grid
// geometry, its exact centroids in leaf order and their voxel keys.  c3h_set_vosch_head chooses it.
// 1 (head_batch): the batched voxel head of voxelize.hip (vh_*) -- a bounds pass over the batch's
// concatenated points, the host's decision per frame (vosch_frames.h), one sort whose runs are the
// voxels, a thread per run -- with two host synchronisations per batch and no launch per frame.
// It leaves the colour columns of dim 137 and dim 1001 to the front: one sparse C3-HLAC pass (117
// or 981 bins) over the whole batch's voxel lists (c3_sparse.hip), launched by front_run.
// 0 (front_head): per frame, in turn, c3h_voxelize (which synchronises the host), the exact
// centroids, the leaf layout and, at dim 137 and 1001, the dense C3-HLAC extract (extract_frames),
// whose columns go straight into the frame's output rows.  What a frame leaves for the front is small: its
// geometry on the host (VfHostFrame), its centroids in leaf order and their voxel keys.  Everything else --
// search grids, normals, RSD, GRSD transitions, columns 0 .. 19 -- runs once per batch over a
// device table of per-frame records.  The single-frame entry points are a batch of one frame in
// two steps: c3h_compute_normals fills the normals' half of the record and runs that stage,
// c3h_extract_grsd / c3h_extract_vosch complete the record and run the rest.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "capi_host.h"

using c3h::fail;

namespace {

enum { kStageNormals = 1, kStageGrsd = 2 };

struct FrontParams {
  float radius;    // the cell of every frame's g (the normals' radius)
  float vp[3];     // kStageNormals: the viewpoint
  float max_dist;  // kStageGrsd: the RSD radius,
  float norm;      //   the factor of the rows
  int dim;         //   and their stride
  // the batched head at dim 137 / 1001: columns 20 .. by the sparse C3-HLAC pass (c3_sparse.hip)
  const uint32_t* c3s_lut = nullptr;  // the colour mode's LUT, or nullptr: no such columns
  int32_t c3s_thr[3] = {0, 0, 0};
};

// RSD radius: max(rsd_radius_search, voxel_size / 2 * sqrt(3)) (grsd_colorCHLAC_tools.hpp:172)
float rsd_max_dist(const c3h_grsd_params* gp, float leaf) {
  return (float)std::max((double)gp->rsd_radius, (double)leaf / 2 * std::sqrt(3.0));
}
// A wide RSD radius (c3h::vf_rsd_wide) gets a search grid of its own radius; the normals are
// already computed, and the RSD's per-bin min/max angles do not depend on the neighbour visiting order

int nbr_grid(c3h_ctx* ctx, float cell, c3h::VfGrid* g) {
  if (c3h::vf_nbr_grid(ctx->info.min_b, ctx->info.max_b, ctx->info.leaf, cell, g) != c3h::kVfOk)
    return fail(ctx, C3H_ERR_RANGE, "normals: more than 2^27 search cells");
  return C3H_OK;
}

int points_ready(c3h_ctx* ctx) {
  if (!ctx->have_grid || !ctx->table_valid)
    return fail(ctx, C3H_ERR_STATE, "compute_normals: needs the points of a c3h_voxelize");
  return C3H_OK;
}

// The normals' half of a frame (the rest of *fr is the caller's): the points of the last
// c3h_voxelize and their search grid
int frame_normals(c3h_ctx* ctx, float radius, c3h::VfHostFrame* fr) {
  fr->gi = ctx->info;
  fr->pts = ctx->vargs.pts;
  fr->n = ctx->vargs.n;
  fr->z_limit = ctx->vargs.z_limit;
  const int rc = nbr_grid(ctx, radius, &fr->g);
  fr->g2 = fr->g;
  return rc;
}

// The GRSD half: the head of extractGRSDSignature21, the voxel keys of its centroids (ctx->dsamp)
// into vkeys (nullptr, a single frame: its kernels run before the next head and read the leaf
// layout itself), the RSD's own grid where the wide rule asks for one
int frame_grsd(c3h_ctx* ctx, const c3h_grsd_params* gp, int32_t* vkeys, c3h::VfHostFrame* fr) {
  int rc = c3h::grsd_frame_head(ctx, gp, fr->sb, &fr->H, &fr->inv_s);
  if (rc != C3H_OK) return rc;
  fr->nc = fr->H > 0 ? ctx->info.n_occ : 0;
  for (int a = 0; a < 3; ++a) fr->off[a] = gp->subdiv > 0 ? gp->offset[a] : 0;
  fr->cent = ctx->dsamp.p;
  fr->vkeys = vkeys;
  fr->g2 = fr->g;
  const float max_dist = rsd_max_dist(gp, ctx->info.leaf);
  if (fr->H > 0 && c3h::vf_rsd_wide(max_dist, fr->g.cell)) {
    rc = nbr_grid(ctx, max_dist, &fr->g2);
    if (rc != C3H_OK) return rc;
  }
  fr->layout = vkeys ? nullptr : ctx->tmp_i32.p;
  if (fr->nc > 0 && vkeys) {
    const int64_t nvox = (int64_t)fr->gi.div_b[0] * fr->gi.div_b[1] * fr->gi.div_b[2];
    HIPCHK(c3h::launch_vf_vox_keys(ctx->tmp_i32.p, nvox, fr->nc, vkeys, ctx->stream));
  }
  return C3H_OK;
}

// The table's last upload has read the host copy, which may change again; the kernels behind
// that upload stay in flight (they read the device copy, in stream order)
int table_wait(c3h_ctx* ctx) {
  if (ctx->vf_up_ev) HIPCHK(hipEventSynchronize(ctx->vf_up_ev));
  return C3H_OK;
}

// The host table for a call of nf frames
int front_begin(c3h_ctx* ctx, int nf, c3h::VfTable** ht) {
  const int rc = table_wait(ctx);
  if (rc != C3H_OK) return rc;
  if (!ctx->vf_htab) HIPCHK(hipHostMalloc(&ctx->vf_htab, sizeof(c3h::VfTable)));
  *ht = ctx->vf_htab;
  memset(*ht, 0, offsetof(c3h::VfTable, fr) + (size_t)nf * sizeof(c3h::VfFrame));
  (*ht)->nf = nf;
  return C3H_OK;
}

// frame j's share of the concatenations (a failed frame: VfHostFrame{}, nothing)
void push_prefixes(c3h::VfTable* ht, int j, const c3h::VfHostFrame& fr) {
  ht->ppre[j + 1] = ht->ppre[j] + fr.n;
  ht->cpre[j + 1] = ht->cpre[j] + fr.g.ncell;
  ht->c2pre[j + 1] = ht->c2pre[j] + fr.g2.ncell;
  ht->vpre[j + 1] = ht->vpre[j] + fr.nc;
  ht->hpre[j + 1] = ht->hpre[j] + fr.H;
}

// info[j] of a frame whose status is st and, where it succeeded, whose host record is fr
void fill_info(c3h_frame_info* fi, int st, const c3h::VfHostFrame& fr, int64_t n_moved) {
  memset(fi, 0, sizeof(*fi));
  fi->status = st;
  if (st < 0) return;
  for (int a = 0; a < 3; ++a) {
    fi->div_b[a] = fr.gi.div_b[a];
    fi->min_b[a] = fr.gi.min_b[a];
    fi->subdiv_b[a] = fr.sb[a];
  }
  fi->n_valid = fr.gi.n_valid;
  fi->n_occ = fr.gi.n_occ;
  fi->n_moved = fr.H > 0 ? (int32_t)n_moved : 0;
}

// The batched head has no single-frame grid to leave: none is held from here on
void drop_single_frame(c3h_ctx* ctx) {
  ctx->have_grid = false;
  ctx->table_valid = false;
  ctx->vcent_valid = false;
  ctx->normals_valid = false;
  ctx->rsd_n = 0;
  ctx->grid_ptr = nullptr;
  ctx->have_feat = false;
  ctx->feat_listed = false;
  ctx->g_valid = false;
  ctx->rows_valid = false;
}

// the points a batch can hold at most (negative counts: the frame fails, none)
int64_t batch_points(const int64_t* n, int nb) {
  int64_t upper = 0;
  for (int j = 0; j < nb; ++j) upper += std::max<int64_t>(n[j], 0);
  return upper;
}

// A batch of nb frames begins: its host table and the buffers every head fills, sized by the
// points it can hold.  who: the entry point's name in the messages.
int batch_begin(c3h_ctx* ctx, const char* who, const int64_t* n, int nb, int on_device, c3h::VfTable** ht) {
  const int64_t upper = batch_points(n, nb);
  if (upper > c3h::kVfMaxPoints) return fail(ctx, C3H_ERR_RANGE, std::string(who) + ": a batch holds 2^32 points or more");
  // the previous batch's launches read the buffers that may grow now
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int rc = front_begin(ctx, nb, ht);
  if (rc != C3H_OK) return rc;
  if (!on_device) ENSURE(ctx->vf_pts, upper);
  ENSURE(ctx->vf_cent, upper);
  ENSURE(ctx->vf_vkeys, upper);
  return C3H_OK;
}

// frame j's record of the table, from its prefixes and the front's buffers (both final).
// grids == false (c3_rows_front): no search grid, RSD type or transition buffer exists; those
// fields stay zero
void fill_record(c3h_ctx* ctx, c3h::VfTable* ht, int j, const c3h::VfHostFrame& fr, bool grids = true) {
  c3h::VfFrame& t = ht->fr[j];
  for (int which = 0; grids && which < 2; ++which) {
    const c3h::VfGrid& vg = which ? fr.g2 : fr.g;
    c3h::NbrGrid& g = which ? t.g2 : t.g;
    g.pts = fr.pts;
    g.n = fr.n;
    g.z_limit = fr.z_limit;
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
  ga.cent = fr.cent;
  ga.nc = fr.nc;
  ga.types = grids ? ctx->vf_types.p + ht->vpre[j] : nullptr;
  ga.trans = grids ? ctx->vf_trans.p + ht->hpre[j] * 36 : nullptr;
  for (int a = 0; a < 3; ++a) {
    ga.div_b[a] = fr.gi.div_b[a];
    ga.min_b[a] = fr.gi.min_b[a];
    ga.off[a] = fr.off[a];
    ga.sb[a] = fr.sb[a];
  }
  ga.leaf = fr.gi.leaf;
  ga.inv_leaf = 1.0f / fr.gi.leaf;
  ga.inv_s = fr.inv_s;
  ga.hist1 = fr.H == 1 ? 1 : 0;
  t.vkeys = fr.vkeys;
  t.layout = fr.layout;
  t.rows = fr.rows;
  t.exist = fr.exist;
}

// The first nb records of the host table to the device; vf_up_ev tells when the host copy is read
int table_upload(c3h_ctx* ctx, const c3h::VfTable* ht, int nb) {
  HIPCHK(hipMemcpyAsync(ctx->vf_tab.p, ht, offsetof(c3h::VfTable, fr) + (size_t)nb * sizeof(c3h::VfFrame),
                        hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->vf_up_ev) HIPCHK(hipEventCreateWithFlags(&ctx->vf_up_ev, hipEventDisableTiming));
  HIPCHK(hipEventRecord(ctx->vf_up_ev, ctx->stream));
  return C3H_OK;
}

// The sparse C3-HLAC pass (c3_sparse.hip) over the uploaded table: columns col0 .. col0 + variant - 1
// of every row, rows of `stride` floats.  pk (packed mode, c3h_internal.h): its rows, ids, cap, base,
// frame0, nf and phases are the caller's, the context's pack buffers are filled in here.
int c3_sparse_run(c3h_ctx* ctx, int64_t vtot, int64_t htot, const uint32_t* lut, const int32_t thr[3], int variant,
                  int stride, int col0, c3h::C3sPack* pk = nullptr) {
  if (pk) {
    ENSURE(ctx->c3s_tile_heads, c3h::c3s_plan_tiles(vtot));
    ENSURE(ctx->c3s_tile_base, c3h::c3s_plan_tiles(vtot) + 1);
    ENSURE(ctx->c3s_multi_slot, c3h::c3s_multi_cap(vtot));
    ENSURE(ctx->c3s_frame_first, c3h::kVfMaxFrames + 1);
    pk->tile_heads = ctx->c3s_tile_heads.p;
    pk->tile_base = ctx->c3s_tile_base.p;
    pk->multi_slot = ctx->c3s_multi_slot.p;
    pk->frame_first = ctx->c3s_frame_first.p;
  }
  ENSURE(ctx->c3s_keys, vtot);
  ENSURE(ctx->c3s_keys2, vtot);
  ENSURE(ctx->c3s_idx, vtot);
  ENSURE(ctx->c3s_idx2, vtot);
  ENSURE(ctx->c3s_cnt, 2);
  ENSURE(ctx->c3s_chunks, c3h::c3s_chunk_cap(vtot, htot));
  ENSURE(ctx->c3s_multi_row, c3h::c3s_multi_cap(vtot));
  ENSURE(ctx->c3s_acc, (size_t)c3h::c3s_multi_cap(vtot) * variant);
  size_t sort_bytes = 0;
  c3h::C3sBufs b{ctx->c3s_keys.p, ctx->c3s_keys2.p, ctx->c3s_idx.p,       ctx->c3s_idx2.p, ctx->c3s_cnt.p,
                 ctx->c3s_chunks.p, ctx->c3s_multi_row.p, ctx->c3s_acc.p, nullptr,         &sort_bytes};
  HIPCHK(c3h::launch_c3_sparse(ctx->vf_tab.p, vtot, htot, b, lut, thr, variant, stride, col0, ctx->stream));
  ENSURE(ctx->c3s_tmp, std::max<size_t>(sort_bytes, 1));
  sort_bytes = ctx->c3s_tmp.n;
  b.tmp = ctx->c3s_tmp.p;
  HIPCHK(c3h::launch_c3_sparse(ctx->vf_tab.p, vtot, htot, b, lut, thr, variant, stride, col0, ctx->stream, pk));
  return C3H_OK;
}

// The front over the nb frames of the host table, whose prefixes are pushed: the buffers of the
// stages, the records, the upload, the launches.  A batch runs both stages at once.  A single
// frame runs them in two calls; nothing the second reserves holds a result of the first.
int front_run(c3h_ctx* ctx, c3h::VfTable* ht, const c3h::VfHostFrame* ff, int nb, int stages, const FrontParams& q) {
  const int64_t ptot = ht->ppre[nb], ctot = ht->cpre[nb], c2tot = ht->c2pre[nb], vtot = ht->vpre[nb], htot = ht->hpre[nb];
  if (ptot == 0) return C3H_OK;
  const bool wide = (stages & kStageGrsd) && vtot > 0 && c3h::vf_rsd_wide(q.max_dist, q.radius);
  int64_t max_cells = 1;
  for (int j = 0; j < nb; ++j) max_cells = std::max(max_cells, std::max(ff[j].g.ncell, ff[j].g2.ncell));
  c3h::VfKey key{};
  if (c3h::vf_key(max_cells, nb, ptot, &key) != c3h::kVfOk)
    return fail(ctx, C3H_ERR_RANGE, "vosch frames: the batch does not fit the composite sort key");
  ENSURE(ctx->vf_tab, 1);
  size_t tb = 0;
  if ((stages & kStageNormals) || wide) {  // a search grid is built
    const size_t kw = key.wide ? 1 : 2;  // keys per 64-bit word
    ENSURE(ctx->vf_keys, ((size_t)ptot + kw - 1) / kw);
    ENSURE(ctx->vf_keys2, ((size_t)ptot + kw - 1) / kw);
    ENSURE(ctx->vf_idx, ptot);
    ENSURE(ctx->vf_idx2, ptot);
    ENSURE(ctx->vf_cstart, std::max(ctot, c2tot));
    ENSURE(ctx->vf_cend, std::max(ctot, c2tot));
    HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 0, key, ptot, ctot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                             ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, nullptr, &tb, ctx->stream));
    ENSURE(ctx->vf_tmp, std::max<size_t>(tb, 1));
    tb = ctx->vf_tmp.n;
  }
  if (stages & kStageNormals) {
    ENSURE(ctx->vf_normals, ptot);
    ENSURE(ctx->vf_dense, c3h::vf_dense_cap(ptot) + 1);
  }
  if (stages & kStageGrsd) {
    ENSURE(ctx->vf_types, vtot);
    ENSURE(ctx->vf_radii, vtot);
    ENSURE(ctx->vf_trans, htot * 36);
  }
  for (int j = 0; j < nb; ++j) fill_record(ctx, ht, j, ff[j]);
  const int up = table_upload(ctx, ht, nb);
  if (up != C3H_OK) return up;
  if (stages & kStageNormals) {
    HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 0, key, ptot, ctot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                             ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, ctx->vf_tmp.p, &tb, ctx->stream));
    const int reach = c3h::vf_reach(q.radius, 1.0f / q.radius);
    if (reach > c3h::kVfMaxReach) return fail(ctx, C3H_ERR_STATE, "vosch frames: internal: normals reach");
    HIPCHK(c3h::launch_vf_normals(ctx->vf_tab.p, nb, key, ptot, ctot, ctx->vf_keys2.p, ctx->vf_dense.p, q.radius, reach, q.vp,
                                  ctx->vf_normals.p, ctx->stream));
  }
  if (!(stages & kStageGrsd)) return C3H_OK;
  if (vtot > 0) {
    const float rsd_cell = wide ? q.max_dist : q.radius;
    if (wide)  // (the normals are done with the first grid: its buffers take the second)
      HIPCHK(c3h::vf_nbr_build(ctx->vf_tab.p, 1, key, ptot, c2tot, ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,
                               ctx->vf_idx2.p, ctx->vf_cstart.p, ctx->vf_cend.p, ctx->vf_tmp.p, &tb, ctx->stream));
    HIPCHK(c3h::launch_vf_rsd(ctx->vf_tab.p, vtot, ctx->vf_normals.p, q.max_dist, c3h::vf_reach(q.max_dist, 1.0f / rsd_cell),
                              ctx->vf_radii.p, ctx->vf_types.p, ctx->stream));
  }
  if (htot > 0) {
    HIPCHK(hipMemsetAsync(ctx->vf_trans.p, 0, (size_t)htot * 36 * 4, ctx->stream));
    HIPCHK(c3h::launch_vf_grsd(ctx->vf_tab.p, vtot, ctx->stream));
    HIPCHK(c3h::launch_vf_rows(ctx->vf_tab.p, htot, ctx->vf_trans.p, q.norm, q.dim, ctx->stream));
  }
  if (q.c3s_lut && htot > 0) return c3_sparse_run(ctx, vtot, htot, q.c3s_lut, q.c3s_thr, q.dim - 20, q.dim, 20);
  return C3H_OK;
}

// NORMALIZE_GRSD = 20 / 26 (grsd_colorCHLAC_tools.h:32) when is_normalize
float grsd_norm(const c3h_grsd_params* gp) { return gp->normalize ? (float)(20.0 / 26) : 1.0f; }

// The C3 part of extractVOSCH (grsd_colorCHLAC_tools.hpp:832-843) on the grid of the last
// c3h_voxelize: its C3-HLAC rows of `variant` columns (ctx->feat, ctx->exist) into columns 20 ..
// of rows of 20 + variant floats.  117: VOSCH.  981: ConVOSCH, always from the f32 rows (fp16
// search precision applies to the search only: the extract's f16-row route is not taken here)
int c3_cols(c3h_ctx* ctx, const c3h_grsd_params* gp, int variant, const int32_t thr[3], int32_t color_mode, int64_t H,
            float* rows) {
  c3h_extract_params e{};
  e.variant = variant;
  for (int a = 0; a < 3; ++a) {
    e.thr[a] = thr[a];
    e.offset[a] = gp->offset[a];
  }
  e.subdiv = gp->subdiv;
  e.color_mode = color_mode;
  const uint32_t* g = ctx->grid_ptr;
  int32_t sb2[3];
  int64_t H2 = 0;
  const bool prec16 = ctx->prec16;
  ctx->prec16 = false;
  const int rc = c3h::extract_frames(ctx, &g, 1, &e, sb2, &H2);
  ctx->prec16 = prec16;
  if (rc != C3H_OK) return rc;
  if (H2 != H) return fail(ctx, C3H_ERR_STATE, "extract_vosch: GRSD / C3 subdivisions differ");
  HIPCHK(c3h::launch_vf_c3_cols(ctx->feat.p, ctx->exist.p, H, variant, 20 + variant, rows, ctx->stream));
  return C3H_OK;
}

// extractGRSDSignature21 (grsd_colorCHLAC_tools.hpp:131-296) of the frame c3h_compute_normals
// left in ctx->vf_one: columns 0 .. 19 of H rows of dim floats in `dest`
int grsd_frames(c3h_ctx* ctx, const c3h_grsd_params* gp, int dim, c3h::DevBuf<float>& dest, int32_t sb[3], int64_t* Hout) {
  if (!ctx->normals_valid) return fail(ctx, C3H_ERR_STATE, "extract_grsd: c3h_compute_normals first");
  c3h::VfHostFrame& fr = ctx->vf_one;
  *Hout = 0;
  ctx->vf_nframes = 0;
  int rc = table_wait(ctx);
  if (rc != C3H_OK) return rc;
  rc = frame_grsd(ctx, gp, nullptr, &fr);
  memcpy(sb, fr.sb, sizeof(fr.sb));
  if (rc != C3H_OK) return rc;
  ENSURE(dest, (size_t)std::max<int64_t>(fr.H, 1) * dim);
  if (fr.H == 0) return C3H_OK;
  fr.rows = dest.p;
  c3h::VfTable* const ht = ctx->vf_htab;
  push_prefixes(ht, 0, fr);
  FrontParams q{};
  q.radius = fr.g.cell;
  q.max_dist = rsd_max_dist(gp, ctx->info.leaf);
  q.norm = grsd_norm(gp);
  q.dim = dim;
  rc = front_run(ctx, ht, &fr, 1, kStageGrsd, q);
  if (rc != C3H_OK) return rc;
  ctx->rsd_n = fr.nc;
  fr.g = fr.g2;  // the cell tables hold the RSD's grid from now on
  *Hout = fr.H;
  return C3H_OK;
}

// One frame of a batch through the single-frame head.  Returns its status (0, or the error the
// single-frame route -- c3h_voxelize, c3h_compute_normals, c3h_extract_vosch / _grsd -- gives);
// on success the frame's centroids, voxel keys and C3 columns are enqueued.
int front_head(c3h_ctx* ctx, const float* pts, int64_t n, int on_device, float leaf, float z_limit,
               const c3h_vosch_params* p, int dim, int64_t row_cap, int64_t p0, int64_t v0, float* rows,
               c3h::VfHostFrame* fr) {
  int rc = c3h_voxelize(ctx, pts, n, on_device, leaf, z_limit, nullptr);
  if (rc == C3H_OK) rc = points_ready(ctx);
  if (rc == C3H_OK) rc = frame_normals(ctx, p->normals_radius, fr);
  if (rc != C3H_OK) return rc;
  fr->rows = rows;
  float inv_s;
  if (c3h::vf_subdivisions(fr->gi.div_b, p->grsd.subdiv, p->grsd.offset, fr->sb, &inv_s) > row_cap)
    return fail(ctx, C3H_ERR_RANGE, "vosch frames: a frame has more rows than row_cap");
  rc = frame_grsd(ctx, &p->grsd, ctx->vf_vkeys.p + v0, fr);
  if (rc != C3H_OK) return rc;
  if (!on_device) {  // fr->pts is ctx->pts, where c3h_voxelize staged the host points: the next frame overwrites them
    HIPCHK(hipMemcpyAsync(ctx->vf_pts.p + p0, ctx->pts.p, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
    fr->pts = ctx->vf_pts.p + p0;
  }
  if (fr->nc > 0) {  // and ctx->dsamp
    HIPCHK(hipMemcpyAsync(ctx->vf_cent.p + v0, ctx->dsamp.p, (size_t)fr->nc * 16, hipMemcpyDeviceToDevice, ctx->stream));
    fr->cent = ctx->vf_cent.p + v0;
  }
  if (dim != 20) return c3_cols(ctx, &p->grsd, dim - 20, p->thr, p->color_mode, fr->H, fr->rows);
  return C3H_OK;
}

static_assert(c3h::vh_status(c3h::kVhGood) == C3H_OK && c3h::vh_status(c3h::kVhArgs) == C3H_ERR_ARG &&
                  c3h::vh_status(c3h::kVhNoPoint) == C3H_ERR_STATE && c3h::vh_status(c3h::kVhRows) == C3H_ERR_RANGE,
              "vh_status speaks the header's codes");

const char* head_reason(int reason) {
  switch (reason) {
    case c3h::kVhArgs: return "c3h_voxelize: bad arguments";
    case c3h::kVhPoints: return "c3h_voxelize: at most 16,777,215 points per call";
    case c3h::kVhBeyond: return "c3h_voxelize: leaf size too small (cell coordinates beyond +-2^20)";
    case c3h::kVhNoPoint: return "compute_normals: needs the points of a c3h_voxelize";
    case c3h::kVhVoxels: return "c3h_voxelize: leaf size too small for int32 voxel indices";
    case c3h::kVhCells: return "normals: more than 2^27 search cells";
    default: return "vosch frames: a frame has more rows than row_cap";
  }
}

// The nb frames of a batch through the batched voxel head (voxelize.hip vh_*): every frame's
// status, info, VfHostFrame and prefixes as nb front_head calls leave them, with two host
// synchronisations for the batch -- the bounds of the frames, then their voxel counts.  The
// centroids and voxel keys of all frames are runs of one sort over the concatenated points; the
// context's single-frame grid, voxeliser state and extract buffers are not used (vh_* buffers).
// dim: the rows' stride.  d_rows: the slot of the batch's first frame.  c3_only (c3_rows_front):
// dim is the C3-HLAC variant; no search grid is sized or checked, and negative thresholds make
// every frame the reference's silent-empty case.  Otherwise the colour columns of dim 137 / 1001
// come from the front's sparse pass (front_run): what the per-frame extract of head 0 refuses of
// the call's colour mode and thresholds is refused here, per frame, with its status and message.
int head_batch(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int nb, int on_device, float leaf, float z_limit,
               const c3h_vosch_params* p, int dim, int64_t row_cap, float* d_rows, const FrontParams& q,
               c3h::VfTable* ht, c3h::VfHostFrame* ff, c3h_frame_info* info, bool c3_only = false) {
  if (!ctx->vh_host) HIPCHK(hipHostMalloc(&ctx->vh_host, sizeof(c3h_ctx::VhHost)));
  c3h_ctx::VhHost* const hh = ctx->vh_host;
  ENSURE(ctx->vh_tab, 2);
  ENSURE(ctx->vh_rec, c3h::kVfMaxFrames);
  ENSURE(ctx->vh_vord, c3h::kVfMaxFrames + 1);
  // ---- the bounds of every frame whose arguments pass
  c3h::VhTable& ta = hh->tab[0];
  memset(&ta, 0, sizeof(ta));
  ta.nf = nb;
  ta.leaf = leaf;
  ta.inv_leaf = 1.0f / leaf;  // c3h_voxelize's
  ta.z_limit = z_limit;
  for (int j = 0; j < nb; ++j) {
    const bool ok = c3h::vh_args_reason(n[j], pts[j] != nullptr) == c3h::kVhGood;
    ta.ppre[j + 1] = ta.ppre[j] + (ok ? n[j] : 0);
    hh->init[j] = hh->back[j] = c3h::vh_rec_init();
  }
  const int64_t ptot0 = ta.ppre[nb];
  for (int j = 0; j < nb; ++j) {
    if (ta.ppre[j + 1] == ta.ppre[j]) continue;
    if (on_device) {
      ta.fr[j].pts = reinterpret_cast<const float4*>(pts[j]);
    } else {  // staged where the front reads it
      HIPCHK(hipMemcpyAsync(ctx->vf_pts.p + ta.ppre[j], pts[j], (size_t)n[j] * 16, hipMemcpyHostToDevice, ctx->stream));
      ta.fr[j].pts = ctx->vf_pts.p + ta.ppre[j];
    }
  }
  if (ptot0 > 0) {
    HIPCHK(hipMemcpyAsync(ctx->vh_rec.p, hh->init, (size_t)nb * sizeof(c3h::VhRec), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->vh_tab.p, &ta, sizeof(ta), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(c3h::launch_vh_bounds(ctx->vh_tab.p, ptot0, ctx->vh_rec.p, ctx->stream));
    HIPCHK(hipMemcpyAsync(hh->back, ctx->vh_rec.p, (size_t)nb * sizeof(c3h::VhRec), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  // ---- the host's decision per frame; the frames that go on, concatenated again
  c3h::VhCall call{};
  call.leaf = leaf;
  call.radius = p->normals_radius;
  call.rsd_dist = q.max_dist;
  call.subdiv = p->grsd.subdiv;
  if (c3_only && (p->thr[0] < 0 || p->thr[1] < 0 || p->thr[2] < 0)) call.subdiv = -1;  // computeFeature (c3_hlac.cpp:398-401)
  for (int a = 0; a < 3; ++a) call.offset[a] = p->grsd.offset[a];
  call.row_cap = row_cap;
  call.no_grids = c3_only ? 1 : 0;
  c3h::VhTable& tb = hh->tab[1];
  tb = ta;
  int reason[c3h::kVfMaxFrames];
  int64_t max_vox = 1;
  for (int j = 0; j < nb; ++j) {
    c3h::VfHostFrame& fr = ff[j];
    fr = c3h::VfHostFrame{};
    c3h::VhFrameGeom gm;
    reason[j] = c3h::vh_frame_decide(n[j], pts[j] != nullptr, hh->back[j], call, &gm);
    tb.fr[j] = c3h::VhFrame{};
    if (reason[j] == c3h::kVhGood) {
      fr.gi.leaf = leaf;
      fr.gi.inv_leaf = 1.0f / leaf;
      for (int a = 0; a < 3; ++a) {
        fr.gi.min_b[a] = gm.min_b[a];
        fr.gi.max_b[a] = gm.max_b[a];
        fr.gi.div_b[a] = gm.div_b[a];
        fr.sb[a] = gm.sb[a];
        fr.off[a] = p->grsd.subdiv > 0 ? p->grsd.offset[a] : 0;
        tb.fr[j].mn[a] = gm.min_b[a];
        tb.fr[j].dv[a] = gm.div_b[a];
      }
      fr.gi.n_valid = gm.n_valid;
      fr.g = gm.g;
      fr.g2 = gm.g2;
      fr.pts = ta.fr[j].pts;
      fr.n = n[j];
      fr.z_limit = z_limit;
      fr.H = gm.H;
      fr.inv_s = gm.inv_s;
      fr.rows = d_rows + (size_t)j * row_cap * dim;
      tb.fr[j].pts = fr.pts;
      max_vox = std::max(max_vox, gm.nvox);
    } else {
      ctx->err = head_reason(reason[j]);
    }
    tb.ppre[j + 1] = tb.ppre[j] + fr.n;
  }
  // ---- keys, the sort, the runs, the emit
  const int64_t ptot = tb.ppre[nb];
  if (ptot > 0) {
    c3h::VfKey key{};
    if (c3h::vh_key(max_vox, nb, ptot, &key) != c3h::kVfOk)
      return fail(ctx, C3H_ERR_RANGE, "vosch frames: the batch does not fit the voxel sort key");
    tb.voxel_bits = key.cell_bits;
    ENSURE(ctx->vf_keys, ptot);  // (a 64-bit word per key: the front's own sorts find the buffers large enough)
    ENSURE(ctx->vf_keys2, ptot);
    ENSURE(ctx->vf_idx, ptot);
    ENSURE(ctx->vf_idx2, ptot);
    ENSURE(ctx->vh_head, ptot);
    ENSURE(ctx->vh_ord, ptot);
    ENSURE(ctx->vh_sums, c3h::scan_blocks(ptot));
    c3h::VhSortBufs sb{ctx->vf_keys.p, ctx->vf_keys2.p, ctx->vf_idx.p,  ctx->vf_idx2.p, ctx->vh_head.p,
                       ctx->vh_sums.p, ctx->vh_ord.p,   ctx->vh_vord.p, nullptr,        0};
    HIPCHK(c3h::launch_vh_voxels(ctx->vh_tab.p + 1, nb, key, ptot, sb, ctx->vf_cent.p, ctx->vf_vkeys.p, ctx->vh_rec.p,
                                 ctx->stream));
    ENSURE(ctx->vf_tmp, std::max<size_t>(sb.tmp_bytes, 1));
    sb.tmp = ctx->vf_tmp.p;
    sb.tmp_bytes = ctx->vf_tmp.n;
    HIPCHK(hipMemcpyAsync(ctx->vh_tab.p + 1, &tb, sizeof(tb), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(c3h::launch_vh_voxels(ctx->vh_tab.p + 1, nb, key, ptot, sb, ctx->vf_cent.p, ctx->vf_vkeys.p, ctx->vh_rec.p,
                                 ctx->stream));
    HIPCHK(hipMemcpyAsync(hh->back, ctx->vh_rec.p, (size_t)nb * sizeof(c3h::VhRec), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  // ---- the frames' centroids and voxel keys (runs' ordinals: frame after frame), status and info
  const bool colour = !c3_only && dim != 20;
  const bool bad_mode = p->color_mode < C3H_COLOR_C3_FLOAT || p->color_mode > C3H_COLOR_CHLAC;
  const bool bad_thr = p->thr[0] < 0 || p->thr[1] < 0 || p->thr[2] < 0;
  int64_t vall = 0;
  for (int j = 0; j < nb; ++j) {
    c3h::VfHostFrame& fr = ff[j];
    int st = c3h::vh_status(reason[j]);
    if (st == C3H_OK) {
      const int64_t n_occ = hh->back[j].n_occ;
      fr.gi.n_occ = n_occ;
      fr.nc = fr.H > 0 ? n_occ : 0;
      fr.cent = ctx->vf_cent.p + vall;
      fr.vkeys = ctx->vf_vkeys.p + vall;
      fr.layout = nullptr;
      vall += n_occ;
    }
    if (st == C3H_OK && colour) {
      // (a frame without rows keeps the status 0 it has always had here at dim 137, where the
      // extract ran only for a frame with rows; at dim 1001, as at head 0, it is refused)
      if (bad_mode && (fr.H > 0 || dim == 1001))
        st = fail(ctx, C3H_ERR_ARG, "c3h_extract: variant must be 981 or 117, color_mode a C3H_COLOR_* value");
      else if (fr.H > 0 && bad_thr)
        st = fail(ctx, C3H_ERR_STATE, "extract_vosch: GRSD / C3 subdivisions differ");
      if (st < 0) {  // no centroid and no row of it goes on (its points are in the sort already: normals only)
        fr.H = 0;
        fr.nc = 0;
        fr.rows = nullptr;
      }
    }
    fill_info(&info[j], st, fr, hh->back[j].n_off);
    push_prefixes(ht, j, fr);
  }
  return C3H_OK;
}

// The front end of both batch entry points: frame i's rows at d_rows + i * row_cap * dim, info[i]
// filled (info != nullptr).  Returns C3H_OK or the error that stopped the call.
int vosch_front(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device, float leaf,
                float z_limit, const c3h_vosch_params* p, int32_t dim, int64_t row_cap, float* d_rows,
                c3h_frame_info* info) {
  HIPCHK(hipSetDevice(ctx->device));
  const int B = std::max(1, std::min(ctx->nbatch, c3h::kVfMaxFrames));
  ctx->vf_nframes = 0;
  if (ctx->vosch_head == 1) drop_single_frame(ctx);
  ctx->vf_n.assign(n, n + nframes);
  ctx->vf_status.assign((size_t)nframes, 0);
  ctx->vf_ppre.assign((size_t)nframes + 1, 0);
  ctx->vf_vpre.assign((size_t)nframes + 1, 0);
  FrontParams q{};
  q.radius = p->normals_radius;
  for (int a = 0; a < 3; ++a) q.vp[a] = p->viewpoint[a];
  q.max_dist = rsd_max_dist(&p->grsd, leaf);
  q.norm = grsd_norm(&p->grsd);
  q.dim = dim;
  if (dim != 20 && ctx->vosch_head == 1 && p->color_mode >= C3H_COLOR_C3_FLOAT && p->color_mode <= C3H_COLOR_CHLAC) {
    q.c3s_lut = ctx->lut.p + 256 * p->color_mode;
    for (int a = 0; a < 3; ++a) q.c3s_thr[a] = p->thr[a];
  }
  std::vector<c3h::VfHostFrame> ff((size_t)B);
  for (int b0 = 0; b0 < nframes; b0 += B) {
    const int nb = std::min(B, nframes - b0);
    c3h::VfTable* ht = nullptr;
    int rc = batch_begin(ctx, "vosch frames", n + b0, nb, on_device, &ht);
    if (rc != C3H_OK) return rc;
    if (ctx->vosch_head == 1) {
      rc = head_batch(ctx, pts + b0, n + b0, nb, on_device, leaf, z_limit, p, dim, row_cap,
                      d_rows + (size_t)b0 * row_cap * dim, q, ht, ff.data(), info + b0);
      if (rc != C3H_OK) return rc;
    }
    for (int j = 0; j < nb; ++j) {
      const int i = b0 + j;
      if (ctx->vosch_head != 1) {
        c3h::VfHostFrame& fr = ff[(size_t)j];
        fr = c3h::VfHostFrame{};
        const int st = front_head(ctx, pts[i], n[i], on_device, leaf, z_limit, p, dim, row_cap, ht->ppre[j], ht->vpre[j],
                                  d_rows + (size_t)i * row_cap * dim, &fr);
        if (st < 0) fr = c3h::VfHostFrame{};  // no points, cells, centroids or rows in the batch
        fill_info(&info[i], st, fr, ctx->n_offcell);
        push_prefixes(ht, j, fr);
      }
      ctx->vf_status[(size_t)i] = info[i].status;
      if (nframes <= B) {
        ctx->vf_ppre[(size_t)i + 1] = ht->ppre[j + 1];
        ctx->vf_vpre[(size_t)i + 1] = ht->vpre[j + 1];
      }
    }
    rc = front_run(ctx, ht, ff.data(), nb, kStageNormals | kStageGrsd, q);
    if (rc != C3H_OK) return rc;
  }
  ctx->vf_nframes = nframes <= B ? nframes : -1;
  return C3H_OK;
}

// The packed mode of c3_rows_front: only the rows that hold a voxel, in the order (frame, row).
// c3h_extract_c3_frames_packed: rows / ids / cap are the caller's (rows == nullptr: the count alone).
// c3h_pca_add_c3_frames (pca != nullptr): per batch the count is read, a buffer of the context is
// sized to it, the rows go to the PCA object's accumulator.
struct PackedCall {
  int64_t cap = 0;
  float* rows = nullptr;
  c3h::C3sPackedRow* ids = nullptr;
  int64_t* frame_first = nullptr;  // host, nframes + 1, may be nullptr
  c3h_pca* pca = nullptr;
  int rotate24 = 0;
  int64_t total = 0;               // out: the rows of the call
  // the batch whose frame_first readback is in flight
  int pend_b0 = 0, pend_nb = 0;
};

// After a wait on the context's stream: the pending batch's packed rows in front of its frames
void packed_take(c3h_ctx* ctx, PackedCall* pc) {
  for (int j = 0; j < pc->pend_nb; ++j)
    if (pc->frame_first) pc->frame_first[pc->pend_b0 + j] = pc->total + ctx->c3s_pack_host[j];
  if (pc->pend_nb) pc->total += ctx->c3s_pack_host[pc->pend_nb];
  pc->pend_nb = 0;
}

// One batch of c3h_pca_add_c3_frames behind its plan: the count, the buffer, the accumulate launches,
// the hand-over.  The PCA's stream waits for the rows (c3s_rows_ev); the context's stream waits,
// before it writes the buffer again, until the SYRK has read them (c3s_read_ev).
int packed_to_pca(c3h_ctx* ctx, PackedCall* pc, c3h::C3sPack* pk, int64_t vtot, int64_t htot, const uint32_t* lut,
                  const int32_t thr[3], int variant) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const int64_t count = ctx->c3s_pack_host[pk->nf];
  pc->pend_nb = 0;
  if (count == 0) return C3H_OK;
  const bool first = !ctx->c3s_rows_ev;
  if (first) {
    HIPCHK(hipEventCreateWithFlags(&ctx->c3s_rows_ev, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->c3s_read_ev, hipEventDisableTiming));
  }
  if (!first) {
    if (ctx->c3s_pca_rows.n < (size_t)count * variant) HIPCHK(hipEventSynchronize(ctx->c3s_read_ev));  // the buffer is freed
    else HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->c3s_read_ev, 0));
  }
  ENSURE(ctx->c3s_pca_rows, (size_t)count * variant);
  pk->rows = ctx->c3s_pca_rows.p;
  pk->phases = c3h::kC3sPackAccum;
  int rc = c3_sparse_run(ctx, vtot, htot, lut, thr, variant, variant, 0, pk);
  if (rc != C3H_OK) return rc;
  hipStream_t ps = c3h::pca_stream(pc->pca);
  HIPCHK(hipEventRecord(ctx->c3s_rows_ev, ctx->stream));
  HIPCHK(hipStreamWaitEvent(ps, ctx->c3s_rows_ev, 0));
  rc = c3h_pca_add_data(pc->pca, ctx->c3s_pca_rows.p, count, variant, variant, pc->rotate24, 1);
  // (recorded whatever add_data returned: the next wait must not meet an event never recorded)
  HIPCHK(hipEventRecord(ctx->c3s_read_ev, ps));
  if (rc != C3H_OK) return fail(ctx, rc, std::string("c3h_pca_add_c3_frames: ") + c3h_pca_last_error(pc->pca));
  pc->total += count;
  return C3H_OK;
}

// c3h_extract_c3_frames: the batched voxel head, then the sparse C3-HLAC pass alone -- frame i's
// rows at d_rows + i * row_cap * variant, its exist values at d_exist + i * row_cap.  No search
// grid, normal, RSD or GRSD buffer is touched.  pc: the packed mode (row_cap INT64_MAX, no d_rows).
int c3_rows_front(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device, float leaf,
                  float z_limit, const c3h_extract_params* e, int64_t row_cap, float* d_rows, int32_t* d_exist,
                  c3h_frame_info* info, PackedCall* pc = nullptr) {
  HIPCHK(hipSetDevice(ctx->device));
  const int B = std::max(1, std::min(ctx->nbatch, c3h::kVfMaxFrames));
  for (int b0 = 0; b0 < nframes; b0 += B)  // (refused before any batch runs)
    if (batch_points(n + b0, std::min(B, nframes - b0)) > c3h::kVfMaxPoints)
      return fail(ctx, C3H_ERR_RANGE, "c3 frames: a batch holds 2^32 points or more");
  ctx->vf_nframes = 0;
  drop_single_frame(ctx);
  const int variant = e->variant;
  c3h_vosch_params p{};
  p.grsd.subdiv = e->subdiv;
  p.normals_radius = leaf;  // (unread: the head sizes no search grid)
  p.color_mode = e->color_mode;
  for (int a = 0; a < 3; ++a) {
    p.grsd.offset[a] = e->offset[a];
    p.thr[a] = e->thr[a];
  }
  FrontParams q{};
  q.dim = variant;
  const uint32_t* lut = ctx->lut.p + 256 * e->color_mode;
  std::vector<c3h::VfHostFrame> ff((size_t)B);
  for (int b0 = 0; b0 < nframes; b0 += B) {
    const int nb = std::min(B, nframes - b0);
    c3h::VfTable* ht = nullptr;
    int rc = batch_begin(ctx, "c3 frames", n + b0, nb, on_device, &ht);
    if (rc != C3H_OK) return rc;
    if (pc) packed_take(ctx, pc);  // (batch_begin's wait also brought the previous batch's count)
    rc = head_batch(ctx, pts + b0, n + b0, nb, on_device, leaf, z_limit, &p, variant, row_cap,
                    pc ? nullptr : d_rows + (size_t)b0 * row_cap * variant, q, ht, ff.data(), info + b0, true);
    if (rc != C3H_OK) return rc;
    const int64_t vtot = ht->vpre[nb], htot = ht->hpre[nb];
    if (htot == 0 || (pc && vtot == 0)) {
      for (int j = 0; pc && pc->frame_first && j < nb; ++j) pc->frame_first[b0 + j] = pc->total;
      continue;
    }
    ENSURE(ctx->vf_tab, 1);
    for (int j = 0; j < nb; ++j) {
      if (pc) ff[(size_t)j].rows = nullptr;  // (no frame has a slot)
      if (d_exist && ff[(size_t)j].H > 0) ff[(size_t)j].exist = d_exist + (size_t)(b0 + j) * row_cap;
      fill_record(ctx, ht, j, ff[(size_t)j], false);
    }
    rc = table_upload(ctx, ht, nb);
    if (rc != C3H_OK) return rc;
    if (!pc) {
      rc = c3_sparse_run(ctx, vtot, htot, lut, p.thr, variant, variant, 0);
      if (rc != C3H_OK) return rc;
      continue;
    }
    if (!ctx->c3s_pack_host) HIPCHK(hipHostMalloc(&ctx->c3s_pack_host, (c3h::kVfMaxFrames + 1) * sizeof(int64_t)));
    c3h::C3sPack pk{};
    pk.rows = pc->rows;
    pk.ids = pc->ids;
    pk.cap = pc->pca ? INT64_MAX : pc->cap;  // (the PCA's buffer is sized to the count: every row has a place)
    pk.base = pc->pca ? 0 : pc->total;
    pk.frame0 = b0;
    pk.nf = nb;
    pk.phases = pc->pca || !pc->rows ? c3h::kC3sPackPlan : c3h::kC3sPackPlan | c3h::kC3sPackAccum;
    rc = c3_sparse_run(ctx, vtot, htot, lut, p.thr, variant, variant, 0, &pk);
    if (rc != C3H_OK) return rc;
    HIPCHK(hipMemcpyAsync(ctx->c3s_pack_host, ctx->c3s_frame_first.p, (size_t)(nb + 1) * sizeof(int64_t),
                          hipMemcpyDeviceToHost, ctx->stream));
    pc->pend_b0 = b0;
    pc->pend_nb = nb;
    if (pc->pca) {
      rc = packed_to_pca(ctx, pc, &pk, vtot, htot, lut, p.thr, variant);
      if (rc != C3H_OK) return rc;
    }
  }
  if (pc) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    packed_take(ctx, pc);
    if (pc->frame_first) pc->frame_first[nframes] = pc->total;
  }
  return C3H_OK;
}

int front_args(c3h_ctx* ctx, const char* who, const float* const* pts, const int64_t* n, int32_t nframes, float leaf,
               const c3h_vosch_params* p, int32_t dim) {
  if (!ctx || !p || nframes < 0 || (nframes > 0 && (!pts || !n))) return C3H_ERR_ARG;
  if (dim != 137 && dim != 1001 && dim != 20)
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": dim must be 137 (VOSCH), 1001 (ConVOSCH) or 20 (GRSD)");
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

// ---- one frame: the points of the last c3h_voxelize -----------------------------------------
int c3h_compute_normals(c3h_ctx* ctx, float radius, const float viewpoint[3]) {
  if (!ctx || !(radius > 0)) return C3H_ERR_ARG;
  QUIESCE(ctx);
  int rc = points_ready(ctx);
  if (rc != C3H_OK) return rc;
  HIPCHK(hipSetDevice(ctx->device));
  ctx->normals_valid = false;
  c3h::VfHostFrame& fr = ctx->vf_one;
  fr = c3h::VfHostFrame{};
  rc = frame_normals(ctx, radius, &fr);
  if (rc != C3H_OK) return rc;
  ctx->vf_nframes = 0;  // the frame takes the buffers of the last batch
  c3h::VfTable* ht = nullptr;
  rc = front_begin(ctx, 1, &ht);
  if (rc != C3H_OK) return rc;
  push_prefixes(ht, 0, fr);
  FrontParams q{};
  q.radius = radius;
  for (int a = 0; a < 3; ++a) q.vp[a] = viewpoint ? viewpoint[a] : 0.0f;
  rc = front_run(ctx, ht, &fr, 1, kStageNormals, q);
  if (rc != C3H_OK) return rc;
  ctx->normals_valid = true;
  return C3H_OK;
}

int c3h_get_normals(c3h_ctx* ctx, float* out, int on_device) {
  if (!ctx || !out) return C3H_ERR_ARG;
  QUIESCE(ctx);
  if (!ctx->normals_valid) return fail(ctx, C3H_ERR_STATE, "get_normals: c3h_compute_normals first");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(out, ctx->vf_normals.p, (size_t)ctx->vargs.n * 16,
                        on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return C3H_OK;
}

int c3h_extract_grsd(c3h_ctx* ctx, const c3h_grsd_params* p, int32_t subdiv_out[3], int64_t* hist_num) {
  if (!ctx || !p) return C3H_ERR_ARG;
  QUIESCE(ctx);
  if (!ctx->have_grid || !ctx->table_valid) return fail(ctx, C3H_ERR_STATE, "extract_grsd: no c3h_voxelize grid");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->have_feat = false;
  ctx->feat_listed = false;
  ctx->g_valid = false;
  ctx->rows_valid = false;
  ctx->exist_gates_rows = false;
  int32_t sb[3];
  int64_t H = 0;
  int rc = grsd_frames(ctx, p, 20, ctx->feat, sb, &H);
  if (rc != C3H_OK) return rc;
  ctx->feat16_pending = false;
  ENSURE(ctx->exist, (size_t)std::max<int64_t>(H, 1));
  if (H > 0) HIPCHK(c3h::launch_exist_rule(ctx->feat.p, H, 20, C3H_EXIST_GRSD, ctx->exist.p, ctx->stream));
  ctx->hist_num = H;
  ctx->feat_dim = 20;
  for (int a = 0; a < 3; ++a) ctx->subdiv_b[a] = sb[a];
  ctx->nframes_feat = 1;
  ctx->feat_sparse = false;
  ctx->have_feat = true;
  if (subdiv_out) memcpy(subdiv_out, sb, sizeof(sb));
  if (hist_num) *hist_num = H;
  return C3H_OK;
}

int c3h_get_rsd(c3h_ctx* ctx, float* radii, int32_t* types, int on_device) {
  if (!ctx) return C3H_ERR_ARG;
  QUIESCE(ctx);
  if (ctx->rsd_n == 0 && !ctx->normals_valid) return fail(ctx, C3H_ERR_STATE, "get_rsd: no RSD computed");
  HIPCHK(hipSetDevice(ctx->device));
  const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (radii && ctx->rsd_n) HIPCHK(hipMemcpyAsync(radii, ctx->vf_radii.p, (size_t)ctx->rsd_n * 8, k, ctx->stream));
  if (types && ctx->rsd_n) HIPCHK(hipMemcpyAsync(types, ctx->vf_types.p, (size_t)ctx->rsd_n * 4, k, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return (int)std::min<int64_t>(ctx->rsd_n, INT32_MAX);
}

// extractVOSCH (grsd_colorCHLAC_tools.hpp:832-843): [GRSD-20 | C3-HLAC-117] per subdivision;
// ConVOSCH (example_GRSD_CCHLAC.cpp): [GRSD-20 | C3-HLAC-981]
static int extract_vosch_rows(c3h_ctx* ctx, const c3h_grsd_params* p, int variant, const int32_t thr[3], int32_t color_mode,
                              int32_t subdiv_out[3], int64_t* hist_num) {
  if (!ctx || !p || !thr) return C3H_ERR_ARG;
  QUIESCE(ctx);
  if (!ctx->have_grid || !ctx->table_valid) return fail(ctx, C3H_ERR_STATE, "extract_vosch: no c3h_voxelize grid");
  HIPCHK(hipSetDevice(ctx->device));
  int32_t sb[3];
  int64_t H = 0;
  int rc = grsd_frames(ctx, p, 20 + variant, ctx->vf_rows, sb, &H);
  if (rc != C3H_OK) return rc;
  rc = c3_cols(ctx, p, variant, thr, color_mode, H, ctx->vf_rows.p);
  if (rc != C3H_OK) return rc;
  std::swap(ctx->feat, ctx->vf_rows);  // (extract_frames left the C3-HLAC rows in feat)
  ctx->feat_dim = 20 + variant;
  ctx->feat_sparse = false;
  ctx->g_valid = false;
  ctx->rows_valid = false;
  ctx->exist_gates_rows = false;
  if (subdiv_out) memcpy(subdiv_out, sb, sizeof(sb));
  if (hist_num) *hist_num = H;
  return C3H_OK;
}

int c3h_extract_vosch(c3h_ctx* ctx, const c3h_grsd_params* p, const int32_t thr[3], int32_t color_mode,
                      int32_t subdiv_out[3], int64_t* hist_num) {
  return extract_vosch_rows(ctx, p, 117, thr, color_mode, subdiv_out, hist_num);
}

int c3h_extract_convosch(c3h_ctx* ctx, const c3h_grsd_params* p, const int32_t thr[3], int32_t color_mode,
                         int32_t subdiv_out[3], int64_t* hist_num) {
  return extract_vosch_rows(ctx, p, 981, thr, color_mode, subdiv_out, hist_num);
}

// ---- a batch of frames ------------------------------------------------------------------------

int c3h_set_vosch_head(c3h_ctx* ctx, int32_t head) {
  if (!ctx || (head != 0 && head != 1)) return C3H_ERR_ARG;
  QUIESCE(ctx);
  ctx->vosch_head = head;
  return C3H_OK;
}

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

int c3h_extract_c3_frames(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device,
                          float leaf, float z_limit, const c3h_extract_params* p, int64_t row_cap, float* d_rows,
                          int32_t* d_exist, c3h_frame_info* info) {
  if (!ctx || !p || nframes < 0 || (nframes > 0 && (!pts || !n))) return C3H_ERR_ARG;
  if ((p->variant != 981 && p->variant != 117) || p->color_mode < C3H_COLOR_C3_FLOAT || p->color_mode > C3H_COLOR_CHLAC)
    return fail(ctx, C3H_ERR_ARG, "c3h_extract_c3_frames: variant must be 981 or 117, color_mode a C3H_COLOR_* value");
  if (!(leaf > 0)) return fail(ctx, C3H_ERR_ARG, "c3h_extract_c3_frames: leaf must be > 0");
  if (row_cap < 1 || (nframes > 0 && !d_rows)) return fail(ctx, C3H_ERR_ARG, "c3h_extract_c3_frames: row_cap / d_rows");
  QUIESCE(ctx);
  std::vector<c3h_frame_info> own;
  if (!info) {
    own.resize((size_t)std::max(nframes, 1));
    info = own.data();
  }
  return c3_rows_front(ctx, pts, n, nframes, on_device, leaf, z_limit, p, row_cap, d_rows, d_exist, info);
}

static_assert(sizeof(c3h_packed_row) == sizeof(c3h::C3sPackedRow) && offsetof(c3h_packed_row, frame) == offsetof(c3h::C3sPackedRow, frame) &&
                  offsetof(c3h_packed_row, exist) == offsetof(c3h::C3sPackedRow, exist) &&
                  offsetof(c3h_packed_row, row) == offsetof(c3h::C3sPackedRow, row),
              "c3h_packed_row is the kernels' id record");

// the whole-call checks of c3h_extract_c3_frames, for the packed entry points too
static int c3_frames_args(c3h_ctx* ctx, const char* who, const float* const* pts, const int64_t* n, int32_t nframes, float leaf,
                          const c3h_extract_params* p) {
  if (!ctx || !p || nframes < 0 || (nframes > 0 && (!pts || !n))) return C3H_ERR_ARG;
  if ((p->variant != 981 && p->variant != 117) || p->color_mode < C3H_COLOR_C3_FLOAT || p->color_mode > C3H_COLOR_CHLAC)
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": variant must be 981 or 117, color_mode a C3H_COLOR_* value");
  if (!(leaf > 0)) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": leaf must be > 0");
  return C3H_OK;
}

int c3h_extract_c3_frames_packed(c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes, int on_device,
                                 float leaf, float z_limit, const c3h_extract_params* p, int64_t packed_cap, float* d_rows,
                                 c3h_packed_row* d_ids, int64_t* n_packed, int64_t* frame_first, c3h_frame_info* info) {
  const char* who = "c3h_extract_c3_frames_packed";
  int rc = c3_frames_args(ctx, who, pts, n, nframes, leaf, p);
  if (rc != C3H_OK) return rc;
  if (!n_packed || packed_cap < 0 || (packed_cap > 0 && !d_rows) || (!d_rows && d_ids))
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": packed_cap / d_rows / n_packed");
  QUIESCE(ctx);
  std::vector<c3h_frame_info> own;
  if (!info) {
    own.resize((size_t)std::max(nframes, 1));
    info = own.data();
  }
  PackedCall pc;
  pc.cap = packed_cap;
  pc.rows = d_rows;
  pc.ids = reinterpret_cast<c3h::C3sPackedRow*>(d_ids);
  pc.frame_first = frame_first;
  *n_packed = 0;
  rc = c3_rows_front(ctx, pts, n, nframes, on_device, leaf, z_limit, p, INT64_MAX, nullptr, nullptr, info, &pc);
  if (rc != C3H_OK) return rc;
  *n_packed = pc.total;
  if (d_rows && pc.total > packed_cap)
    return fail(ctx, C3H_ERR_RANGE, std::string(who) + ": more rows than packed_cap (n_packed holds the number needed)");
  return C3H_OK;
}

int c3h_pca_add_c3_frames(c3h_pca* pca, c3h_ctx* ctx, const float* const* pts, const int64_t* n, int32_t nframes,
                          int on_device, float leaf, float z_limit, const c3h_extract_params* p, int32_t rotate24,
                          int64_t* rows_added, c3h_frame_info* info) {
  const char* who = "c3h_pca_add_c3_frames";
  if (!pca) return C3H_ERR_ARG;
  int rc = c3_frames_args(ctx, who, pts, n, nframes, leaf, p);
  if (rc != C3H_OK) {
    if (ctx) c3h::pca_set_error(pca, std::string(who) + ": " + c3h_last_error(ctx));
    return rc;
  }
  if (!rows_added) return fail(ctx, C3H_ERR_ARG, std::string(who) + ": rows_added");
  *rows_added = 0;
  if (c3h::pca_device(pca) != ctx->device) {
    c3h::pca_set_error(pca, std::string(who) + ": the PCA object and the context are on different devices");
    return fail(ctx, C3H_ERR_ARG, std::string(who) + ": the PCA object and the context are on different devices");
  }
  // what c3h_pca_add_data refuses (a differing F, rotate24 at 117) it refuses here, with its status
  // and message, before anything is enqueued: an add of no rows
  rc = c3h_pca_add_data(pca, nullptr, 0, p->variant, p->variant, rotate24, 1);
  if (rc != C3H_OK) return fail(ctx, rc, std::string(who) + ": " + c3h_pca_last_error(pca));
  QUIESCE(ctx);
  std::vector<c3h_frame_info> own;
  if (!info) {
    own.resize((size_t)std::max(nframes, 1));
    info = own.data();
  }
  PackedCall pc;
  pc.pca = pca;
  pc.rotate24 = rotate24;
  rc = c3_rows_front(ctx, pts, n, nframes, on_device, leaf, z_limit, p, INT64_MAX, nullptr, nullptr, info, &pc);
  *rows_added = pc.total;
  if (rc != C3H_OK) c3h::pca_set_error(pca, c3h_last_error(ctx));
  return rc;
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
                                dim == 20 ? C3H_EXIST_GRSD : C3H_EXIST_VOSCH, range, exist_threshold, rotate, d_out);
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
