"""The tick's score role on the f32 matrix cores (score_tick_mfma_body) against the VALU score
role (score_list_body) and the float64 oracle.

64^3 grids, leaf 0.04, C3-HLAC-117, box 2x2x2, exist threshold 10, the pipelined
c3h_run_frames at 8 frames per batch over 5 full batches and a ragged one of 3, so every one
of the four buffer sets is reused.  The frames cycle over four resident grids, shifted by one
after four batches: a buffer set's slot then holds another grid than the last time, and the
gate's sparse -1 fill meets stale scores of another layout.

  scene   synth.kinect_scene voxelised: 408 of 3,375 positions pass at S = 4
          (12 full list chunks and a ragged one of 24)
  rolled  the same, rolled 5 cells in x
  dense   5 % random occupancy, random colours: every position passes (106 chunks over 16
          score workgroups: the chunk loop)
  empty   no voxel: nothing passes (the n == 0 path)

(D, M, r): the bench's (100, 10, 20), one pass of 7 column tiles; (20, 7, 12), 84 columns,
models straddling tile edges, 2 model groups; (40, 2, 40), a model wider than a tile;
(20, 3, 5), one group, on the matrix cores only with engine 2; (20, 20, 12), 240 columns
that do not fit one pass (4 passes of 5 models); the bench's again at S = 8, 343 positions
(10 full chunks and one of 23 in fewer workgroups than the 16 of a frame).

Engine 1 (c3h_set_score_engine) keeps the VALU role; engines 0 and 2 must give every
frame's detection record and the last frame's score array bit for bit (the matrix-core
projection is the same k-ordered fmaf chain).  Engine 1's records are checked against the
float64 oracle: scores within 1e-5 relative, another position only on a tie within 2e-5;
the last frame's scores() has the oracle's gated-out pattern and is within 1e-5."""
import numpy as np
import pytest

import c3hlac
import pyoracle as po
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu

RTOL = 1e-5
G, LEAF, F, BOX, EXIST = 64, 0.04, 117, (2, 2, 2), 10
BATCH, NFR = 8, 5 * 8 + 3
NAMES = ["scene", "rolled", "dense", "empty"]
# (D, M, r, S)
CASES = [(100, 10, 20, 4), (20, 7, 12, 4), (40, 2, 40, 4), (20, 3, 5, 4), (20, 20, 12, 4), (100, 10, 20, 8)]
# the oracle's count of positions passing the gate, per S and grid
NPASS = {4: dict(scene=408, dense=3375, empty=0), 8: dict(dense=343, empty=0)}


@pytest.fixture(scope="module")
def grids(ctx):
    """The four resident grids and, per S, the oracle's exact features and exist counts."""
    import torch
    gi = ctx.voxelize(synth.kinect_scene(60_000, grid=G, leaf=LEAF, seed=synth.BASE_SEED + 1), LEAF)
    assert list(gi.div_b) == [G] * 3
    scene = ctx.grid().reshape(G, G, G).copy()
    rng = np.random.default_rng(5)
    occ = rng.random(G ** 3) < 0.05
    dense = np.where(occ, (1 << 24) | rng.integers(0, 1 << 24, G ** 3, dtype=np.uint32), 0).astype(np.uint32)
    words = dict(scene=scene.reshape(-1), rolled=np.ascontiguousarray(np.roll(scene, 5, axis=2)).reshape(-1),
                 dense=dense, empty=np.zeros(G ** 3, np.uint32))
    d_words = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in words.items()}
    torch.cuda.synchronize()
    feats = {}
    for s in sorted({c[3] for c in CASES}):
        for k, w in words.items():
            g, layout, cloud = po.grid_inputs(w, (G,) * 3, LEAF)
            fe, sb, _ = po.c3hlac(g, layout, cloud, F, THR, LEAF, s, exact=True)
            feats[s, k] = (fe, sb, po.exist(fe))
    return dict(d_words=d_words, feats=feats)


_REFS = {}


def _refs(grids, case):
    """The float64 oracle's scores of the four grids for one (D, M, r, S): computed once."""
    if case not in _REFS:
        D, M, r, s = case
        axis_t, var, axis_q = synth.random_bases(F, D, M, r, seed=synth.BASE_SEED + 3)
        ap = synth.whiten(axis_t, var)
        ref = {}
        for k in NAMES:
            fe, sb, ex = grids["feats"][s, k]
            _, _, sc = po.search(sb, fe, ex, ap, axis_q, BOX, 1, EXIST, dbl=True, want_scores=True)
            shape = tuple(int(n) - b + 1 for n, b in zip(sb[::-1], BOX))  # (z, y, x) positions
            ref[k] = (sc.reshape(M, -1), shape)
        for k, n in NPASS[s].items():
            assert int((ref[k][0][0] >= 0).sum()) == n, (k, s)
        _REFS[case] = dict(bases=(axis_t, var, axis_q), ref=ref)
    return _REFS[case]


def _check_det(rec, scores_f64, shape, tag):
    """rec: (M, 3) int64 c3h_det words of one frame; scores_f64: (M, P) oracle scores of the
    single mode (box 2x2x2), P in (z, y, x) scan order."""
    ze, ye, xe = shape
    for m in range(rec.shape[0]):
        s = float(rec[m, 0:1].view(np.float64)[0])
        x, y, z, mode = (int(v) for v in rec[m, 1:3].view(np.int32))
        ref = scores_f64[m]
        best = int(np.argmax(ref))  # first maximum in scan order = searchPart's strict '>'
        assert mode == 0, (tag, m, mode)
        p = (z * ye + y) * xe + x
        assert abs(s - ref[p]) <= RTOL * ref[p], (tag, m, s, ref[p])
        if p != best:  # only a tie within tolerance may pick another position
            assert ref[p] >= ref[best] * (1 - 2 * RTOL), (tag, m, (x, y, z), np.unravel_index(best, shape))


def _frame_name(i, cycle):
    return cycle[(i + i // (4 * BATCH)) % 4]  # shifted by one once every buffer set was used


@pytest.mark.parametrize("last", ["dense", "scene"])
@pytest.mark.parametrize("case", CASES, ids=["D%d_M%d_r%d_S%d" % c for c in CASES])
def test_tick_score_engines_agree_and_match_oracle(ctx, grids, case, last):
    import torch
    D, M, r, s = case
    refs = _refs(grids, case)
    cycle = {"dense": ["empty", "scene", "rolled", "dense"], "scene": ["rolled", "dense", "empty", "scene"]}[last]
    names = [_frame_name(i, cycle) for i in range(NFR)]
    assert names[-1] == last and set(names[:BATCH]) == set(NAMES)
    assert any(names[i] != names[i + 4 * BATCH] for i in range(NFR - 4 * BATCH))  # a set's slot changes grid
    ptrs = np.array([grids["d_words"][k].data_ptr() for k in names], np.uint64)
    ctx.search_setup(*refs["bases"])
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)
    got, scores = {}, {}
    try:
        for engine in (1, 0, 2):
            ctx.set_score_engine(engine)
            d_out = torch.zeros((NFR, M * 3), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.timing(c3hlac.timing_mask("pipeline"))
            ctx.kernel_times(reset=True)
            ctx.run_frames(ptrs, (G,) * 3, (0, 0, 0), LEAF, F, THR, s, BOX, EXIST, True, d_out.data_ptr())
            ctx.synchronize()
            kt = ctx.kernel_times(reset=True)
            ctx.timing(False)
            assert kt["pipeline"][1] == NFR, ("frames through the tick", engine, kt["pipeline"])
            got[engine] = d_out.cpu().numpy().reshape(NFR, M, 3)
            scores[engine] = ctx.scores()
    finally:
        ctx.timing(False)
        ctx.set_score_engine(0)
        ctx.set_batch(32)
    # engines agree bit for bit: every record (the empty frames' included), the last frame's scores
    for engine in (0, 2):
        bad = np.flatnonzero((got[engine] != got[1]).any(axis=(1, 2)))
        assert bad.size == 0, ("records", engine, bad[:8].tolist(), [names[i] for i in bad[:8]])
        assert np.array_equal(scores[engine], scores[1]), ("scores", engine)
    # engine 1 against the float64 oracle
    for i, k in enumerate(names):
        if k != "empty":
            sc, shape = refs["ref"][k]
            _check_det(got[1][i], sc, shape, "%s frame %d (%s)" % (case, i, k))
    sc = refs["ref"][last][0].reshape(-1)
    gs = scores[1]
    assert gs.shape == sc.shape
    assert np.array_equal(gs < 0, sc < 0)
    ok = sc > 0
    np.testing.assert_allclose(gs[ok], sc[ok], rtol=RTOL)
