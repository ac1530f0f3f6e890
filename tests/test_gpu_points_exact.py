"""Points-in exact-centroid pass (voxb_scatter / voxb_bucket / voxb_exact / point_fixup) at
its caps and on face points, against oracle/pyoracle.py.

A voxel whose fp32 centroid (sequential sum * (1/n), PCL 1.0) lies in another cell than its
points takes that cell as subdivision and neighbour base (c3_hlac.cpp:349-377).  The batch
path flags candidates, buckets their points, sums them in input order and repairs the
subdivisions that lose or gain a moved voxel.  Every frame here is built so that this
repair carries the result, and the CPU-side conditions below are asserted on the oracle
alone before a frame is trusted:

- status-0 frames: <= 4,096 occupied voxels, <= 65,536 points, 20..256 moved voxels (no cap
  can trip whatever the device's flag rule does);
- power: the oracle's features with every centroid replaced by its own cell centre differ
  from the correct ones in >= 10 subdivision rows (the one row there is at S = 0);
- interactions (from the oracle's moved list): a subdivision touched by >= 2 moved voxels,
  a moved voxel whose centroid cell holds another voxel, two moved voxels in adjacent
  cells, a moved voxel that crosses a subdivision border;
- by hand: a moved voxel into an otherwise empty subdivision, a subdivision whose only
  voxel moves out, a voxel in cell 0 of x whose centroid cell is -1.

The generator is test_gpu_parity.py::test_points_on_cell_boundaries' with a face fraction:
each point in a random cell of a G^3 block, per axis with probability ff on the cell's lower
face or one ulp beside it, else at 0.1-0.9 of the cell; an optional whole-cell shift.

CPU-side counts of the chosen seeds (leaf 0.01; moved / occupied voxels / subdivisions
touched by >= 2 moved voxels / moved onto an occupied cell / adjacent moved pairs / border
crossings / rows differing from the uncorrected reference):

    frame (test)                         moved   occ  >=2   onto  pairs  cross  rows
    G 24, 4,000 pts, ff .15, S 6 (1, 5)     96  3243   40     16     10     51    72
    same, S 5 offset (2,1,0) (1)           100  3324   33     16     11     33    77
    G 12, 1,400 pts, ff .3, one subdiv (1)  36   954    1     18      5      -     1
    G 24, 2,400 pts, shift +20,000 (2)      93  2040   32      7     13     17    60
    G 24, 2,400 pts, shift -20,000 (2)      79  2036   18     10      6      3    45
    80 x 750 points (3)                     47   480   16      2      4     11    34
    65/66/64/63-point buckets (3)           26   480    8      1      1      6    22
    good A, B, C (4)                  95/98/83  ~2940  47/43/27 21/19/17 7/14/2 67/59/43 78/77/77

In the 80 x 750 frame 22 of the 80 voxels land in another centroid cell when their points
are summed in a shuffled order.  The cap frames: X1 364 moved voxels (3,461 occupied, 4,000
points), X2 4,200 single-point voxels with the point on a face, X3 100 voxels x 700 face
points (70,052 points, 152 voxels).

Feature rows: the same cloud as four one-frame batches puts one copy on the context (buffer
set 0 of the pipeline's four); ctx.exist() / ctx.features() then show the batch's rows in
the canvas's subdivision layout.  Usable: the rows and the exist gate compare exactly with the
oracle's in every status-0 case here.

Outcome on the code as it was: every case passed except two, both fixed (DESIGN.md
section 8, round 14).  981-S16-one (a canvas of one searched subdivision) gave other
records than the single-frame path: point_fixup dropped a moved voxel whose centroid cell
lies below cell 0, which the reference counts when there is one subdivision
(fix_centre_sub).  981-S0: c3h_run_point_frames returned C3H_ERR_STATE ("the canvas does
not fit the pipeline"): without subdivisions the reference's SearchObj::setData returns
early and the pipeline had no batch without a search.  Such a batch now runs its C3 stage
and fixup alone; its records are the fresh lists, subdiv_b is (0, 0, 0) as the oracle's,
and its one feature row is compared like the others."""
import functools

import numpy as np
import pytest

import c3hlac
import pyoracle as po
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

f32 = np.float32
LEAF = 0.01
LEAF32 = f32(LEAF)
INV32 = f32(1) / LEAF32
CANVAS = (32, 32, 32)
M, R, D, RANK, BOX, EXIST = 8, 6, 24, 8, (1, 1, 1), 1
RTOL = 1e-5
FLAG_CAP, BUCKET_CAP, MOVED_CAP = 4096, 65536, 256  # kVbFlagCap, kVbBucketCap, kVbMovedCap

# (variant, S, offset, colour mode) of test 1
CASES = [(117, 6, (0, 0, 0), c3hlac.COLOR_C3_DOUBLE),
         (981, 6, (0, 0, 0), c3hlac.COLOR_C3_DOUBLE),
         (117, 5, (2, 1, 0), c3hlac.COLOR_C3_DOUBLE),
         (981, 0, (0, 0, 0), c3hlac.COLOR_C3_DOUBLE),
         (117, 6, (0, 0, 0), c3hlac.COLOR_CHLAC),
         (981, 16, (0, 0, 0), c3hlac.COLOR_C3_DOUBLE)]  # hist_num == 1 with a search (see FACE_ONE)
CASE_IDS = ["117-S6", "981-S6", "117-S5-off210", "981-S0", "117-S6-chlac", "981-S16-one"]


# ---- clouds ---------------------------------------------------------------------------
def _cells(xyz):
    """The voxel grid's cell of each point (getVoxelGrid: floor(p * inverse_leaf_size))."""
    return np.floor(np.asarray(xyz, f32) * INV32).astype(np.int64)


def _with_colour(xyz, rng):
    col = rng.integers(0, 256, (len(xyz), 3))
    rgb = synth.pack_rgb(col[:, 0], col[:, 1], col[:, 2])
    return np.ascontiguousarray(np.concatenate([np.asarray(xyz, f32), rgb[:, None]], 1), f32)


def _face_cloud(rng, n, g, ff, shift=0):
    """(n, 3) float32: the generator of the module docstring."""
    cells = rng.integers(0, g, (n, 3)) + shift
    face = (cells.astype(f32) * LEAF32).astype(f32)
    ulp = rng.integers(-1, 2, (n, 3))
    face = np.where(ulp == 0, face, np.nextafter(face, np.where(ulp < 0, -np.inf, np.inf).astype(f32)))
    inner = ((cells + 0.1 + 0.8 * rng.random((n, 3))) * np.float64(LEAF32)).astype(f32)
    return np.where(rng.random((n, 3)) < ff, face, inner).astype(f32)


def _centroid_cells(x, nmax):
    """Per n = 1..nmax: the cell of the fp32 centroid of n copies of the coordinate x
    (sequential sum * (1/n), cell = floor(c / leaf): the oracle's PCL 1.0 arithmetic)."""
    s = f32(0)
    out = []
    for n in range(1, nmax + 1):
        s = f32(s + x)
        out.append(int(np.floor(f32(s * (f32(1) / f32(n))) / LEAF32)))
    return out


@functools.lru_cache(maxsize=None)
def _edge_coord(cell, direction):
    """(x, n): n copies of the float32 x lie in `cell` and their centroid in cell + direction
    (far from the origin only the rounding of a long sum carries a centroid that far)."""
    x = f32(np.float64(cell + (1 if direction > 0 else 0)) * np.float64(LEAF32))
    inward = f32(-np.inf if direction > 0 else np.inf)
    for _ in range(8):  # onto the last float32 of the cell on that side
        if int(np.floor(x * INV32)) == cell and int(np.floor(np.nextafter(x, -inward) * INV32)) != cell:
            break
        x = np.nextafter(x, inward if int(np.floor(x * INV32)) != cell else -inward)
    assert int(np.floor(x * INV32)) == cell, (cell, direction)
    best = None
    for k in range(4):
        cc = _centroid_cells(x, 400)
        hit = [n for n in range(2, 401) if cc[n - 1] == cell + direction]
        if hit and (best is None or hit[0] < best[1]):
            best = (x, hit[0])
        x = np.nextafter(x, inward)
        if int(np.floor(x * INV32)) != cell:
            break
    assert best is not None, "no rounding centroid for cell %d direction %d" % (cell, direction)
    return best


def _edge_voxel(cell, axis, direction):
    """Points (identical coordinates, so their order does not matter) of one voxel in the
    absolute `cell` whose centroid cell is one further along `axis`."""
    x, n = _edge_coord(int(cell[axis]), direction)
    p = ((np.asarray(cell) + 0.5) * np.float64(LEAF32)).astype(f32)
    p[axis] = x
    assert (_cells(p[None]) == np.asarray(cell)).all()
    return np.repeat(p[None], n, 0)


def _several(S, off, extent):
    """The frame has the three subdivisions per axis that the hand-built voxels use."""
    return S > 0 and extent >= 3 * S + max(off)


def _sub_of(rel, S, off):
    """Subdivision of canvas / frame cells (rel: (..., 3) offsets from min_b); -1 = no centre."""
    t = np.asarray(rel) - np.asarray(off)
    return np.where(t >= 0, t // S, -1)


def _face_frame(seed, n, g, ff, shift, S, off):
    """A generator cloud plus the three hand-built voxels; subdivisions E (2,1,1) and Q
    (1,2,2) are cleared (and the cells around them), V1 moves from (1,1,1) into the empty E, V2 is Q's only voxel and
    moves out into (2,2,2), V3 sits in cell 0 of x and its centroid in cell -1."""
    rng = np.random.default_rng(seed)
    xyz = _face_cloud(rng, n, g, ff, shift)
    cells = _cells(xyz)
    lo = cells.min(0)
    rel = cells - lo
    special = []
    v3 = np.array([0, 3, 4])
    drop = (rel == v3).all(1)
    if _several(S, off, g + 1):
        o = np.asarray(off)
        for sub in ((2, 1, 1), (1, 2, 2)):  # cleared with a shell of one cell: nothing moves in
            first = o + np.array(sub) * S
            drop |= ((rel >= first - 1) & (rel <= first + S)).all(1)
        v1 = o + np.array([2 * S - 1, S + S // 2, S + S // 2])
        v2 = o + np.array([2 * S - 1, 2 * S + S // 2, 2 * S + S // 2])
        drop |= (rel == v1).all(1)
        special += [_edge_voxel(lo + v1, 0, +1), _edge_voxel(lo + v2, 0, +1)]
    special.append(_edge_voxel(lo + v3, 0, -1))
    xyz = np.concatenate([xyz[~drop]] + special, 0)
    xyz = xyz[rng.permutation(len(xyz))]
    return _with_colour(xyz, rng)


def _seq_cells(P):
    """Centroid cells of the point sets P (..., m, 3): fp32 sequential sum * (1/m),
    floor(c / leaf) -- the oracle's arithmetic, vectorised over the leading axes."""
    s = np.zeros(P.shape[:-2] + (3,), f32)
    for j in range(P.shape[-2]):
        s = (s + P[..., j, :]).astype(f32)
    return np.floor((s * (f32(1) / f32(P.shape[-2]))).astype(f32) / LEAF32).astype(np.int64)


def _bucket_frame(seed, sizes, nfill, spread=0.0):
    """len(sizes) voxels of sizes[v] points dealt round-robin over the input; nfill single-
    point filler voxels first.  Per voxel and axis the coordinates lie in a band of four
    ulps just below the upper face of the cell.  The rounding of a long fp32 sum is worth
    up to ~200 ulps of the centroid, so the band sits 1 + d ulps (d < 256, 2e-4 of a cell)
    below the face, d chosen where the centroid in input order tips from the next cell back
    into the voxel's own: the last additions decide the cell.  Points that differ by a few
    ulps round alike in a long sum whatever their order, so a fraction `spread` of the
    coordinates lies up to 1,024 ulps (0.0008 of a cell) below the face instead: which of
    them meet the sum while it is small and which while it is large changes its rounding,
    and with it the centroid's cell."""
    rng = np.random.default_rng(seed)
    nv = len(sizes)
    lin = rng.choice(18 ** 3, nv, replace=False)
    vc = np.stack([lin % 18, (lin // 18) % 18, lin // 324], 1) + 2  # cells 2..19
    top = np.empty((nv, 3), f32)
    for v in range(nv):
        for a in range(3):
            x = f32(np.float64(vc[v, a] + 1) * np.float64(LEAF32))
            while int(np.floor(x * INV32)) != vc[v, a]:
                x = np.nextafter(x, f32(-np.inf))
            top[v, a] = x  # the last float32 of the cell
    ds = np.arange(256, dtype=np.int32)
    per_voxel = []
    for v in range(nv):
        k = rng.integers(0, 4, (sizes[v], 3), dtype=np.int32)
        wide = rng.random(k.shape) < spread
        k = np.where(wide, rng.integers(0, 1024, k.shape, dtype=np.int32), k)
        band = (~wide).astype(np.int32)
        bits = top[v].view(np.int32)[None, None, :] - k[None, :, :] - ds[:, None, None] * band[None]  # floats > 0
        up = _seq_cells(bits.view(f32)) == vc[v] + 1  # (256, 3): the centroid in the next cell
        d = np.zeros(3, np.int32)
        for a in range(3):
            tip = np.flatnonzero(up[:-1, a] & ~up[1:, a])  # cell + 1 at d, the own cell at d + 1
            if tip.size:
                d[a] = tip[0] + (v + a) % 2
        per_voxel.append((top[v].view(np.int32)[None, :] - k - d[None, :] * band).view(f32))
    vid = np.concatenate([np.full(s, v) for v, s in enumerate(sizes)])
    pos = np.concatenate([np.arange(s) for s in sizes])
    order = np.argsort(pos, kind="stable")  # round-robin: every bucket spans the whole input
    vid = vid[order]
    xyz = np.concatenate(per_voxel, 0)[order]  # a voxel's points keep their order
    assert (_cells(xyz) == vc[vid]).all()
    fc = rng.choice(24 ** 3, nfill, replace=False)
    fc = np.stack([fc % 24, (fc // 24) % 24, fc // 576], 1)
    fc = fc[~(fc[:, None, :] == vc[None, :, :]).all(2).any(1)]
    fc = np.concatenate([fc, [[0, 0, 0], [23, 23, 23]]], 0)
    fill = ((fc + 0.2 + 0.6 * rng.random(fc.shape)) * np.float64(LEAF32)).astype(f32)
    return _with_colour(np.concatenate([fill, xyz], 0), rng), vc, vid, len(fill)


# ---- the oracle's view of a frame -----------------------------------------------------
class Ref:
    pass


def _moved_list(g, layout, cloud):
    d = np.array(g.div_b)
    lo = np.array(g.min_b)
    occ = np.flatnonzero(layout >= 0)
    own = np.stack([occ % d[0], (occ // d[0]) % d[1], occ // (d[0] * d[1])], 1)
    assert np.array_equal(layout[occ], np.arange(len(occ)))
    cc = np.floor(cloud[:, :3] / LEAF32).astype(np.int64) - lo  # floor(c / leaf), fp32 division
    return own, cc, (cc != own).any(1)


def _reference(pts, variant, S, off, cm):
    """Geometry, moved list, exact features, exist, float64 scores and rank lists."""
    po.set_voxel_semantics(True)
    r = Ref()
    g, layout, cloud = po.voxelize(pts, LEAF)
    r.g, r.layout, r.cloud = g, layout, cloud
    r.own, r.cc, r.moved = _moved_list(g, layout, cloud)
    r.n_moved = int(r.moved.sum())
    r.fe, sb, hn = po.c3hlac(g, layout, cloud, variant, THR, LEAF, S, off, cm, exact=True)
    assert hn >= 0, hn  # no centroid past the last subdivision
    r.sb = tuple(sb)  # (0, 0, 0) without subdivisions
    r.ex = po.exist(r.fe)
    # the uncorrected reference: every centroid at its own cell's centre
    flat = cloud.copy()
    flat[:, :3] = ((r.own + np.array(g.min_b) + 0.5) * np.float64(LEAF32)).astype(f32)
    assert not _moved_list(g, layout, flat)[2].any()
    fu, _, _ = po.c3hlac(g, layout, flat, variant, THR, LEAF, S, off, cm, exact=True)
    r.rows_differ = int((fu != r.fe).any(1).sum())
    return r


def _scores(r, bases, rank=RANK, box=BOX):
    axis_t, var, axis_q = bases
    if min(r.sb) < 1:  # no subdivisions: SearchObj::setData returns early, the lists stay fresh
        return po.Lists(axis_q.shape[0], rank), np.zeros((axis_q.shape[0], 0))
    ap = synth.whiten(axis_t, var)
    L, _, sc = po.search(r.sb, r.fe, r.ex, ap, axis_q, box, rank, EXIST, dbl=True, want_scores=True)
    return L, sc.reshape(axis_q.shape[0], -1)


def _interactions(r, S, off):
    """(subdivisions touched by >= 2 moved voxels, moved onto an occupied cell, adjacent
    moved pairs, subdivision border crossings, into an empty subdivision, singleton out)."""
    own, cc = r.own[r.moved], r.cc[r.moved]
    d = np.array(r.g.div_b)
    inside = ((cc >= 0) & (cc < d)).all(1)
    lin = (cc[inside] * np.array([1, d[0], d[0] * d[1]])).sum(1)
    onto = int((r.layout[lin] >= 0).sum())
    diff = np.abs(own[:, None, :] - own[None, :, :]).max(2)
    pairs = int(((diff == 1).sum()) // 2)
    if not _several(S, off, int(d.min())):  # one subdivision: every moved voxel touches it
        return int(r.n_moved >= 2), onto, pairs, 0, 0, 0
    key = lambda s: tuple(int(v) for v in s)  # noqa: E731
    so, sc_ = _sub_of(own, S, off), _sub_of(cc, S, off)
    touched = {}
    for a, b in zip(so, sc_):
        for s in {key(a), key(b)}:
            if min(s) >= 0:
                touched[s] = touched.get(s, 0) + 1
    cross = int((so != sc_).any(1).sum())
    centres = {}  # voxels per subdivision as the reference counts them
    for s in _sub_of(r.cc, S, off):
        centres[key(s)] = centres.get(key(s), 0) + 1
    owners = {}  # and by their own cell
    for s in _sub_of(r.own, S, off):
        owners[key(s)] = owners.get(key(s), 0) + 1
    into_empty = sum(1 for a, b in zip(so, sc_) if key(a) != key(b) and min(key(b)) >= 0 and
                     owners.get(key(b), 0) == 0 and centres[key(b)] == 1)
    single_out = sum(1 for a, b in zip(so, sc_) if key(a) != key(b) and min(key(a)) >= 0 and
                     owners[key(a)] == 1 and centres.get(key(a), 0) == 0)
    return sum(1 for v in touched.values() if v >= 2), onto, pairs, cross, into_empty, single_out


def _assert_batched_frame(pts, r, S, off, hand=True):
    """The CPU-side conditions of a frame that must stay batched and exercise the fixup."""
    assert r.g.n_occ <= FLAG_CAP and len(pts) <= BUCKET_CAP, (r.g.n_occ, len(pts))
    assert 20 <= r.n_moved <= MOVED_CAP, r.n_moved
    several = _several(S, off, min(r.g.div_b))
    assert r.rows_differ >= (10 if several else 1), r.rows_differ
    multi, onto, pairs, cross, into_empty, single_out = _interactions(r, S, off)
    assert multi >= 1 and onto >= 1 and pairs >= 1, (multi, onto, pairs)
    if several:
        assert cross >= 1, cross
    if hand:
        if several:
            assert into_empty >= 1 and single_out >= 1, (into_empty, single_out)
        m = r.moved & (r.own[:, 0] == 0) & (r.cc[:, 0] == -1)
        assert m.any()  # cell 0 -> centroid cell -1
    return (r.n_moved, int(r.g.n_occ), multi, onto, pairs, cross, r.rows_differ)


# ---- the device's view ----------------------------------------------------------------
@pytest.fixture(scope="module")
def bases():
    return {F: synth.random_bases(F, D, M, R, seed=synth.BASE_SEED + 140 + F) for F in (117, 981)}


@pytest.fixture
def pctx(ctx):
    ctx.set_pipeline(True)
    ctx.set_remove_overlap(False)
    try:
        yield ctx
    finally:
        ctx.set_remove_overlap(False)
        ctx.set_rank(1)
        ctx.set_batch(32)


def _single(ctx, dev_pts, variant, S, off, cm, rank=RANK, box=BOX):
    ctx.voxelize(dev_pts, LEAF)
    ctx.extract(variant, THR, S, off, cm)
    ctx.set_rank(rank)
    lists, _ = ctx.search(box, EXIST)
    return lists.copy()


def _run(ctx, dev_frames, variant, S, off, cm, rank=RANK, box=BOX, canvas=CANVAS):
    import torch
    d_out = torch.zeros((len(dev_frames), M * rank * 3), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    _, info = ctx.run_point_frames(dev_frames, LEAF, canvas, variant, THR, S, box, EXIST, True, d_out,
                                   offset=off, color_mode=cm)
    return d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(dev_frames), M, rank), info


def _to_dev(pts):
    import torch
    return torch.from_numpy(pts).to("cuda:0")


def _check_info(info, r, tag):
    assert info["status"] == 0, (tag, info)
    assert info["n_moved"] == r.n_moved, (tag, info["n_moved"], r.n_moved)
    assert info["n_occ"] == r.g.n_occ and info["n_valid"] == r.g.n_valid, (tag, info)
    assert list(info["div_b"]) == list(r.g.div_b) and list(info["min_b"]) == list(r.g.min_b), (tag, info)
    assert tuple(info["subdiv_b"]) == r.sb, (tag, info["subdiv_b"], r.sb)


def _check_scores(got, L, sc, sb, tag):
    """Records (M, rank) against the float64 oracle: the score within RTOL of the oracle's at
    the reported position; another position than the oracle's record only on a tie within
    tolerance (test_gpu_points.py's rule, per rank)."""
    xe, ye = sb[0] - BOX[0] + 1, sb[1] - BOX[1] + 1
    rank = got.shape[1]
    for m in range(got.shape[0]):
        for k in range(rank):
            e = got[m, k]
            o = m * rank + k
            if L.score[o] <= 0:  # fewer gated positions than ranks: the cleared record
                assert float(e["score"]) == 0.0, (tag, m, k, e)
                continue
            assert int(e["mode"]) == 0
            p = (int(e["z"]) * ye + int(e["y"])) * xe + int(e["x"])
            s = float(e["score"])
            assert abs(s - sc[m, p]) <= RTOL * sc[m, p], (tag, m, k, s, sc[m, p])
            q = (int(L.z[o]) * ye + int(L.y[o])) * xe + int(L.x[o])
            if p != q:
                assert sc[m, p] >= sc[m, q] * (1 - 2 * RTOL), (tag, m, k, p, q)


def _canvas_rows(r, S, off, canvas):
    """The oracle's exist and feature rows in the canvas's subdivision layout."""
    if S <= 0:
        return r.ex, r.fe
    csb = [int(np.ceil(f32(c - o) * f32(1.0 / S))) for c, o in zip(canvas, off)]
    ex = np.zeros(csb[0] * csb[1] * csb[2], np.int32)
    fe = np.zeros((ex.size, r.fe.shape[1]), f32)
    x, y, z = np.meshgrid(np.arange(r.sb[0]), np.arange(r.sb[1]), np.arange(r.sb[2]), indexing="ij")
    src = (x + r.sb[0] * (y + r.sb[1] * z)).ravel()
    dst = (x + csb[0] * (y + csb[1] * z)).ravel()
    ex[dst] = r.ex[src]
    fe[dst] = r.fe[src]
    return ex, fe


def _check_frame(ctx, pts, r, bases, variant, S, off, cm, other, tag, canvas=CANVAS):
    """One frame through the batch: info, records (single-frame path bit for bit, float64
    oracle within RTOL) and, as four one-frame batches, its exist and feature rows."""
    dev = _to_dev(pts)
    ctx.search_setup(*bases[variant])
    ref = _single(ctx, dev, variant, S, off, cm)
    ctx.set_rank(RANK)
    ctx.set_batch(8)
    got, info = _run(ctx, [dev], variant, S, off, cm, canvas=canvas)
    _check_info(info[0], r, tag)
    assert np.array_equal(got[0], ref), (tag, got[0], ref)
    L, sc = _scores(r, bases[variant])
    _check_scores(got[0], L, sc, r.sb, tag)
    # the rows: leftover state first (another cloud on the single-frame path), then four
    # one-frame batches -- one lands on the context's own buffer set
    _single(ctx, other, variant, S, off, cm)
    ctx.set_rank(RANK)
    ctx.set_batch(1)
    got4, info4 = _run(ctx, [dev] * 4, variant, S, off, cm, canvas=canvas)
    for i in range(4):
        _check_info(info4[i], r, tag)
        assert np.array_equal(got4[i], ref), (tag, i)
    ctx._refresh()
    ex, fe = _canvas_rows(r, S, off, canvas)
    gex = ctx.exist()
    assert gex.shape == ex.shape, (tag, gex.shape, ex.shape)
    bad = np.flatnonzero(gex != ex)
    assert bad.size == 0, (tag, "exist", bad.size, bad[:8].tolist(), gex[bad[:8]].tolist(), ex[bad[:8]].tolist())
    gf = ctx.features()
    assert gf.shape == fe.shape, (tag, gf.shape, fe.shape)
    bad = np.flatnonzero((gf != fe).any(1))
    assert bad.size == 0, (tag, "features", bad.size, bad[:8].tolist())


@functools.lru_cache(maxsize=None)
def _other_cloud():
    rng = np.random.default_rng(77)
    return _with_colour(_face_cloud(rng, 3000, 28, 0.0), rng)


# ---- 1. face-heavy frames stay batched and are exact -----------------------------------
FACE = dict(seed=1401, n=4000, g=24, ff=0.15)
# one subdivision (computeC3HLAC's hist_num == 1 rule: no centre test, offsets ignored): the
# tick takes it as one tile only up to 16 cells per axis.  S = 0 is the issue's case; the
# reference runs no search without subdivisions (SearchObj::setData returns early), so
# S = 16 on the same canvas is the single subdivision that is searched
FACE_ONE = dict(seed=1405, n=1400, g=12, ff=0.3)
CANVAS_ONE = (16, 16, 16)


@functools.lru_cache(maxsize=None)
def _face_case(seed, n, g, ff, shift, variant, S, off, cm):
    pts = _face_frame(seed, n, g, ff, shift, S, off)
    r = _reference(pts, variant, S, off, cm)
    r.counts = _assert_batched_frame(pts, r, S, off)
    return pts, r


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_face_heavy_frames_stay_batched_and_are_exact(pctx, bases, case):
    """981-S0 and 981-S16-one: one histogram, which the tick takes as one tile only up to 16
    cells per axis, so both run a 13^3 frame (36 moved of 954 voxels) on a 16^3 canvas.
    Without subdivisions the reference runs no search: the records are the fresh lists and
    the feature row carries the check."""
    variant, S, off, cm = case
    fr, canvas = (FACE, CANVAS) if S in (5, 6) else (FACE_ONE, CANVAS_ONE)
    pts, r = _face_case(fr["seed"], fr["n"], fr["g"], fr["ff"], 0, variant, S, off, cm)
    print("counts", case, r.counts)
    other = _other_cloud()
    if canvas == CANVAS_ONE:
        other = other[(_cells(other[:, :3]) < 14).all(1)]
    _check_frame(pctx, pts, r, bases, variant, S, off, cm, _to_dev(other), str(case), canvas)


# ---- 2. far from the origin ------------------------------------------------------------
@pytest.mark.parametrize("shift", [20000, -20000])
def test_far_from_the_origin(pctx, bases, shift):
    """cmag = 20,000 cells: eps = (count + 4) * cmag * 2^-22 decides which voxels are flagged."""
    variant, S, off, cm = CASES[0]
    pts, r = _face_case(1402, 2400, 24, 0.15, shift, variant, S, off, cm)
    assert len(pts) <= 3000
    print("counts", shift, r.counts)
    other = _other_cloud().copy()
    other[:, :3] += f32(shift * LEAF)
    _check_frame(pctx, pts, r, bases, variant, S, off, cm, _to_dev(other), "shift %d" % shift)


# ---- 3. large and scattered buckets ----------------------------------------------------
def _order_sensitive(pts, vid, nfill, nv):
    """Voxels whose fp32 sequential centroid lands in another cell when summed in a shuffled
    order than in input order."""
    rng = np.random.default_rng(3)
    xyz = pts[nfill:, :3]
    n = 0
    for v in range(nv):
        p = xyz[vid == v]
        n += int((_seq_cells(p) != _seq_cells(p[rng.permutation(len(p))])).any())
    return n


@functools.lru_cache(maxsize=None)
def _bucket_case(which):
    variant, S, off, cm = CASES[0]
    if which == "large":  # 80 x 750 points: the shell sort at every gap, buckets over 4 chunks
        sizes = [750] * 80
        pts, vc, vid, nfill = _bucket_frame(1403, sizes, 400, spread=0.05)
        assert len(pts) <= BUCKET_CAP and len(pts) > 3 * 16384
        assert _order_sensitive(pts, vid, nfill, len(sizes)) >= 10
    else:  # the first sizes past the LDS sort, and the last ones inside it
        sizes = [65] * 30 + [66] * 30 + [64] * 10 + [63] * 10
        pts, vc, vid, nfill = _bucket_frame(1404, sizes, 400)
    r = _reference(pts, variant, S, off, cm)
    r.counts = _assert_batched_frame(pts, r, S, off, hand=False)
    return pts, r


@pytest.mark.parametrize("which", ["large", "lds_edge"])
def test_large_and_scattered_buckets(pctx, bases, which):
    variant, S, off, cm = CASES[0]
    pts, r = _bucket_case(which)
    print("counts", which, r.counts)
    _check_frame(pctx, pts, r, bases, variant, S, off, cm, _to_dev(_other_cloud()), which)


# ---- 4. the three caps, next to healthy frames -----------------------------------------
@functools.lru_cache(maxsize=None)
def _cap_frames():
    variant, S, off, cm = CASES[0]
    good = [_face_case(1410 + i, 3600, 24, 0.15, 0, variant, S, off, cm) for i in range(3)]
    # X1: more moved voxels than kVbMovedCap
    rng = np.random.default_rng(1420)
    x1 = _with_colour(_face_cloud(rng, 4000, 24, 0.6), rng)
    g, layout, cloud = po.voxelize(x1, LEAF)
    assert _moved_list(g, layout, cloud)[2].sum() > MOVED_CAP and g.n_occ <= FLAG_CAP and len(x1) <= BUCKET_CAP
    # X2: more than kVbFlagCap voxels that hold a point exactly on a face (margin 0)
    lin = rng.choice(28 ** 3, 4200, replace=False)
    c = np.stack([lin % 28, (lin // 28) % 28, lin // 784], 1) + 1
    p = ((c + 0.2 + 0.6 * rng.random(c.shape)) * np.float64(LEAF32)).astype(f32)
    p[:, 0] = (c[:, 0].astype(f32) * LEAF32).astype(f32)
    on_face = _cells(p)[:, 0] == c[:, 0]
    p[~on_face, 0] = np.nextafter(p[~on_face, 0], f32(np.inf))
    assert (_cells(p) == c).all() and (_cells(np.nextafter(p, f32(-np.inf)))[:, 0] == c[:, 0] - 1).all()
    x2 = _with_colour(p, rng)
    assert po.voxelize(x2, LEAF)[0].n_occ >= 4200
    # X3: 100 flagged voxels, more than kVbBucketCap of their points
    x3 = _bucket_frame(1421, [700] * 100, 50)[0]
    assert len(x3) > BUCKET_CAP and po.voxelize(x3, LEAF)[0].n_occ <= FLAG_CAP
    return good, [x1, x2, x3]


def test_caps_next_to_healthy_frames(pctx, bases):
    variant, S, off, cm = CASES[0]
    good, bad = _cap_frames()
    a, b, c = (_to_dev(g[0]) for g in good)
    x1, x2, x3 = (_to_dev(x) for x in bad)
    frames = [a, x1, b, x2, x3, c]
    gi, xi = [0, 2, 5], [1, 3, 4]
    pctx.search_setup(*bases[variant])
    single = [_single(pctx, f, variant, S, off, cm) for f in frames]
    pctx.set_rank(RANK)
    pctx.set_batch(8)
    alone = [_run(pctx, [frames[i]], variant, S, off, cm) for i in gi]
    got, info = _run(pctx, frames, variant, S, off, cm)
    assert list(info["status"]) == [0, 1, 0, 1, 1, 0], info["status"]
    for i in xi:
        assert np.array_equal(got[i], single[i]), (i, got[i], single[i])
    for j, i in enumerate(gi):
        _check_info(info[i], good[j][1], "good %d" % j)
        assert np.array_equal(got[i], alone[j][0][0]) and np.array_equal(got[i], single[i]), i
        assert info[i] == alone[j][1][0], (i, info[i], alone[j][1][0])
    got2, info2 = _run(pctx, frames, variant, S, off, cm)  # nothing of the overflow survives
    assert np.array_equal(got2, got) and np.array_equal(info2, info)
    got3, info3 = _run(pctx, [a, b, c], variant, S, off, cm)
    assert np.array_equal(got3, got[gi]) and np.array_equal(info3, info[gi])


# ---- 5. ranks above 1 and removeOverlap on a moved frame -------------------------------
def test_rank4_remove_overlap_on_a_moved_frame(pctx, bases):
    variant, S, off, cm = CASES[0]
    pts, r = _face_case(FACE["seed"], FACE["n"], FACE["g"], FACE["ff"], 0, variant, S, off, cm)
    dev = _to_dev(pts)
    box = (2, 2, 2)
    pctx.search_setup(*bases[variant])
    ref = c3hlac.remove_overlap(_single(pctx, dev, variant, S, off, cm, rank=4, box=box), box)
    assert (ref["score"] > 0).sum() > M  # more than the maxima survive
    pctx.set_rank(4)
    pctx.set_batch(8)
    pctx.set_remove_overlap(True)
    got, info = _run(pctx, [dev, dev], variant, S, off, cm, rank=4, box=box)
    assert list(info["status"]) == [0, 0] and (info["n_moved"] == r.n_moved).all(), info
    for i in range(2):
        assert np.array_equal(got[i], ref), (i, got[i], ref)
