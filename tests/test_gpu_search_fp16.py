"""The fp16 search precision (c3h_set_search_precision(ctx, 1)) pinned to np_ref.scores_f16 /
compress_f16: the kernels' documented roundings (power-of-two scale, operands rounded to
f16) with float64 sums, so what is left is the matrix instruction's f32 accumulation order
and the tolerance is F16_REF_RTOL (a few 1e-6, measured in test_search_fp16_ref_cpu.py)
instead of the 2e-3 that separates f16 rounding from the float64 oracle.  The models are
np_ref.flat_bases (every basis column weighs the same), so a column credited to the wrong
model, a dropped k tail or a lost lane half moves scores by orders of magnitude more.

Projection: score_mfma_f16s_kernel (r >= 16) and score_mfma_f16_kernel (r < 16) over the
shape table of search_fp16_cases.py -- every KQ from 1 to 10, D < 16, D > 128, r = 16,
r % 4 != 0, uneven model groups, six modes, modes that do not fit, 0 / 1 / 33 passing
positions, more positions than one workgroup step.  Compress: compress_f16_kernel's f32-row
body on the sparse row list (L1, L2), its f16-row body on a dense extract (L3), and the
D > 128 route where the compress stays f32 (L2 at D = 132)."""
import numpy as np
import pytest

import np_ref as npr
from c3hlac import synth
from conftest import THR

import search_fp16_cases as fc
from test_gpu_parity import _assert_replay_matches

pytestmark = pytest.mark.gpu

BOX = (2, 2, 2)


def _search(ctx, fp16, box, rank, thr, rotate=True):
    """One single-frame search on the matrix cores -> lists, scores, G, exist."""
    ctx.set_score_engine(2)
    ctx.set_search_precision(fp16)
    try:
        ctx.set_rank(rank)
        lists, _ = ctx.search(box, thr, rotate=rotate)
        return lists.copy(), ctx.scores().copy(), ctx.compressed().copy(), ctx.exist().copy()
    finally:
        ctx.set_search_precision(False)
        ctx.set_score_engine(0)


def _where(ref, i):
    """Flat score index -> (mode, model, position) for failure messages."""
    for mode, xe, ye, sc in ref:
        if i < sc.size:
            return mode, i // sc.shape[1], i % sc.shape[1]
        i -= sc.size
    return None


def _check_rank1(lists, ref, tag):
    """Rank 1 = the first maximum over every mode in scan order: the record names the
    reference's argmax, or a position tying it within the tolerance; no passing position
    leaves the record empty."""
    rtol = npr.F16_REF_RTOL
    for m in range(lists.shape[0]):
        e = lists[m, 0]
        best = max([float(sc[m].max()) for _, _, _, sc in ref] + [0.0])
        if best <= 0:
            assert (float(e["score"]), int(e["x"]), int(e["y"]), int(e["z"])) == (0.0, 0, 0, 0), (tag, m)
            continue
        hit = [(xe, ye, sc) for mode, xe, ye, sc in ref if mode == int(e["mode"])]
        assert hit, (tag, m, int(e["mode"]))
        xe, ye, sc = hit[0]
        v = sc[m, int(e["x"]) + xe * (int(e["y"]) + ye * int(e["z"]))]
        assert abs(float(e["score"]) - v) <= rtol * v, (tag, m, float(e["score"]), v)
        assert v >= best * (1 - 2 * rtol), (tag, m, v, best)


def _check_scores(tag, s16, s32, sb, G, ex, feat, fexist, ap, axis_q, box, thr, rotate=True, fmax=None):
    """The score assertions of one fp16 search -> the reference's per-mode scores."""
    ref = npr.scores_f16(sb, G, ex, axis_q, box, thr, rotate)
    r = fc.flat(ref)
    ok = r > 0
    assert np.array_equal(s16 > 0, ok), (tag, int((s16 > 0).sum()), int(ok.sum()))
    assert not np.isnan(s16).any()
    if ok.any():
        dev = np.abs(s16[ok] - r[ok]) / r[ok]
        i = int(np.flatnonzero(ok)[np.argmax(dev)])
        rf = fc.flat(npr.scores_f16(sb, G, ex, axis_q, box, thr, rotate, flush_subnormals=True))
        devf = float((np.abs(s16[ok] - rf[ok]) / rf[ok]).max())
        print("%s: %d passing, max |dev| / ref %.3e (flush variant %.3e)" % (tag, int(ok.sum()), dev.max(), devf))
        assert dev.max() <= npr.F16_REF_RTOL, (tag, float(dev.max()), "at (mode, model, position)", _where(ref, i),
                                               float(s16[i]), float(r[i]), "flush variant", devf)
        assert not np.array_equal(s16, s32), tag  # the f16 path really ran
    assert np.array_equal(s32 > 0, ok), tag
    s64 = fc.flat(npr.scores(sb, feat, fexist, ap, axis_q, box, thr, rotate, fmax=fmax))
    assert np.array_equal(s64 > 0, ok), tag
    exc = fc.contract_excess(s16[ok], s64[ok])
    print("%s: contract against float64 %.2f of its bound" % (tag, exc))
    assert exc <= 1.0, (tag, exc)
    return ref


def _run_case(ctx, tag, sb, feat, exist, axis_t, var, axis_q, box, thr, rotate=True, count=None):
    ctx.set_features(feat, sb, exist=exist)
    ctx.search_setup(axis_t, var, axis_q)
    ap = synth.whiten(axis_t, var)
    _, s32, _, _ = _search(ctx, False, box, 1, thr, rotate)
    lists, s16, G, ex = _search(ctx, True, box, 1, thr, rotate)
    assert np.array_equal(ex, exist)
    ref = _check_scores(tag, s16, s32, sb, G, ex, feat, exist, ap, axis_q, box, thr, rotate)
    if count is not None:
        assert int((s16 > 0).sum()) == count * axis_q.shape[0], tag
    _check_rank1(lists, ref, tag)
    lists4, s16b, _, _ = _search(ctx, True, box, 4, thr, rotate)
    assert np.array_equal(s16b, s16), tag
    _assert_replay_matches(ctx, box, 4, lists4, rotate=rotate)
    return ref


@pytest.mark.parametrize("shape", fc.TABLE)
def test_projection_shapes(ctx, shape):
    feat, exist, axis_t, var, axis_q = fc.inputs(shape)
    thr = fc.median_thr(exist, fc.SB, BOX)
    _run_case(ctx, "%s box 2 2 2" % (shape,), fc.SB, feat, exist, axis_t, var, axis_q, BOX, thr)


EDGE_SHAPES = [(100, 5, 70), (100, 10, 13)]


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("box,nmodes", [((1, 2, 3), 6), ((12, 1, 2), 2)])
def test_rotation_modes(ctx, shape, box, nmodes):
    """Six modes in one list (entries of every mode in each 32-lane set), and a box with one
    side 12: only the two modes with the 12 along x fit (13, 11, 9)."""
    feat, exist, axis_t, var, axis_q = fc.inputs(shape)
    thr = fc.median_thr(exist, fc.SB, box)
    ref = _run_case(ctx, "%s box %s" % (shape, box), fc.SB, feat, exist, axis_t, var, axis_q, box, thr)
    assert len(ref) == nmodes
    assert all((sc > 0).any() for _, _, _, sc in ref)


@pytest.mark.parametrize("shape", EDGE_SHAPES)
@pytest.mark.parametrize("count", [1, 33, 0])
def test_exact_passing_counts(ctx, shape, count):
    """Partial 32-lane sets; an empty list leaves no positive score and empty records."""
    D, M, r = shape
    feat, exist, thr = fc.exact_rows(D, 5, count)
    axis_t, var, axis_q = fc.bases(D, M, r, 5)
    _run_case(ctx, "%s exactly %d" % (shape, count), fc.SB, feat, exist, axis_t, var, axis_q, BOX, thr,
              count=count)


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_many_positions(ctx, shape):
    """A (40, 30, 20) canvas: thousands of passing positions, every wave of every workgroup
    loaded (a workgroup step covers 256 of the list at r >= 16, 128 below)."""
    D, M, r = shape
    sb = (40, 30, 20)
    feat, exist = fc.rows(D, 4030, sb)
    axis_t, var, axis_q = fc.bases(D, M, r, 4030)
    thr = fc.median_thr(exist, sb, BOX)
    ref = _run_case(ctx, "%s canvas" % (shape,), sb, feat, exist, axis_t, var, axis_q, BOX, thr)
    assert int((ref[0][3][0] > 0).sum()) > 256


def test_decaying_bases_subnormal_operands(ctx):
    """synth.random_bases' models at the production shape: their rows decay to 0.85^34.5, so
    many basis entries are f16 subnormals -- the reference keeps them, and so must the
    matrix instruction (flushing them moves scores by more than the tolerance:
    test_search_fp16_ref_cpu.py::test_flush_subnormals_is_visible)."""
    feat, exist, axis_t, var, _ = fc.inputs((100, 5, 70))
    axis_q = synth.random_bases(117, 100, 5, 70, seed=9)[2]
    thr = fc.median_thr(exist, fc.SB, BOX)
    _run_case(ctx, "decaying bases", fc.SB, feat, exist, axis_t, var, axis_q, BOX, thr)


# ---------------------------------------------------------------- the f16 compress
# compress_f16_kernel runs from 65,536 subdivisions (kCompressMfmaRows), so these use real
# extracts: |compressed() - G_ref| <= bound on rows with exist > 0, then the score
# assertions on the GPU's G.

@pytest.fixture(scope="module")
def kinect256(ctx):
    return synth.kinect_scene(1_000_000, grid=256, leaf=0.01, seed=synth.BASE_SEED + 256)


def _check_compress(tag, G, ex, feat, ap, fmax=None):
    G_ref, bound = npr.compress_f16(feat, ap, fmax)
    rows = ex > 0
    err = np.abs(G[rows] - G_ref[rows])
    assert (bound[rows] > 0).all()
    print("%s: %d rows, max |dG| / bound %.3f" % (tag, int(rows.sum()), (err / bound[rows]).max()))
    assert (err <= bound[rows]).all(), (tag, float((err / bound[rows]).max()))
    assert (err > 0).any(), tag  # f32 sums of f16 products, not the float64 reference itself


def _extract_case(ctx, tag, variant, D, M, r, use_fmax, seed, thr=100):
    sb, H = ctx.subdiv, ctx.hist_num
    fe, ex = ctx.features(), ctx.exist()
    axis_t, var, _ = synth.random_bases(variant, D, 1, 1, seed=seed)
    axis_q = npr.flat_bases(D, M, r, seed + 1)
    ap = synth.whiten(axis_t, var)
    fmax = (fe.max(0) * np.float32(0.8)).astype(np.float32) if use_fmax else None
    ctx.search_setup(axis_t, var, axis_q, feature_max=fmax)
    _, s32, G32, _ = _search(ctx, False, BOX, 1, thr)
    lists, s16, G, ex16 = _search(ctx, True, BOX, 1, thr)
    assert np.array_equal(ex16, ex)
    ref = _check_scores(tag, s16, s32, sb, G, ex, fe, ex, ap, axis_q, BOX, thr, fmax=fmax)
    assert int((ref[0][3][0] > 0).sum()) > 100
    _check_rank1(lists, ref, tag)
    return fe, ex, ap, fmax, G, G32


def test_compress_l1_sparse_rows_117_fmax(ctx, kinect256):
    """Sparse row list with a ragged last 128-row block; Fp16 = 128 (a zero k tail of 11);
    normalised values above 1 and the v == max -> 1 rule."""
    ctx.voxelize(kinect256, 0.01)
    sb, H = ctx.extract(117, THR, 6)
    assert sb == (43, 43, 43) and H >= 65536
    fe, ex, ap, fmax, G, G32 = _extract_case(ctx, "L1", 117, 100, 3, 20, True, 611)
    assert int((ex > 0).sum()) % 128 != 0
    assert (fe[ex > 0] > fmax[None, :]).any()  # normalised values above 1
    _check_compress("L1", G, ex, fe, ap, fmax)
    assert not np.array_equal(G[ex > 0], G32[ex > 0])  # the f16 compress really ran


def test_compress_l2_981_all_columns_then_f32_route(ctx, kinect256):
    """D = 128: all 128 columns live, Fp16 = 992 (the last 64-wide chunk half full).  Then
    D = 132: no f16 axis exists beyond 128 columns, so the compress is the f32 one (G bit for
    bit the fp32 precision's) followed by the f16 projection."""
    ctx.voxelize(kinect256, 0.01)
    sb, H = ctx.extract(981, THR, 6)
    assert H >= 65536
    fe, ex, ap, _, G, G32 = _extract_case(ctx, "L2 D=128", 981, 128, 2, 33, False, 622)
    _check_compress("L2 D=128", G, ex, fe, ap)
    assert not np.array_equal(G[ex > 0], G32[ex > 0])
    ctx.extract(981, THR, 6)
    fe, ex, ap, _, G, G32 = _extract_case(ctx, "L2 D=132", 981, 132, 2, 33, False, 633)
    assert np.array_equal(G[ex > 0], G32[ex > 0])


def test_compress_l3_f16_rows_dense(ctx):
    """Precision set before the extract of a dense grid of >= 65,536 subdivisions: the C3
    body writes f16 rows and the compress' f16-row body reads them (and, every row being
    listed, takes them in memory order).  123^3 at S = 3 is 41^3 = 68,921 subdivisions, the
    smallest dense grid at a subdivision side the matrix-core C3 body is tested at."""
    Gd, S = 123, 3
    rng = np.random.default_rng(123)
    words = rng.integers(0, 1 << 24, size=Gd ** 3, dtype=np.uint32) | np.uint32(1 << 24)
    ctx.set_grid(words, (Gd,) * 3, leaf=0.01)
    sb, H = ctx.extract(981, THR, S)
    assert sb == (41, 41, 41) and H >= 65536
    fe32 = ctx.features()
    ctx.set_search_precision(True)
    try:
        ctx.extract(981, THR, S)
        axis_t, var, _ = synth.random_bases(981, 100, 1, 1, seed=644)
        axis_q = npr.flat_bases(100, 2, 20, 645)
        ap = synth.whiten(axis_t, var)
        ctx.search_setup(axis_t, var, axis_q)
        ctx.set_score_engine(2)
        ctx.set_rank(1)
        lists, _ = ctx.search(BOX, 100)
        s16, G, ex = ctx.scores().copy(), ctx.compressed().copy(), ctx.exist().copy()
        fe16 = ctx.features()
    finally:
        ctx.set_search_precision(False)
        ctx.set_score_engine(0)
    assert np.array_equal(fe16, fe32.astype(np.float16).astype(np.float32))  # the f16-row body ran
    assert not np.array_equal(fe16, fe32)
    assert (ex > 0).all()
    _check_compress("L3", G, ex, fe16, ap)
    ctx.set_features(fe32, sb, exist=ex)
    _, s32, _, _ = _search(ctx, False, BOX, 1, 100)
    ref = _check_scores("L3", s16, s32, sb, G, ex, fe32, ex, ap, axis_q, BOX, 100)
    _check_rank1(lists, ref, "L3")
