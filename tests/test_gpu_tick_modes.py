"""The pipelined tick at rank 1 off the cubic box: several search modes through the tick's own
argmax (order_base, pstart, md[].mode), modes that do not fit the subdivisions, rotate off,
feature_max in the tick's compress role and a D that is no multiple of 4 -- against the
float64 oracle, the lanes and the single-frame path.

C3-HLAC-117, leaf 0.04, exist threshold 10, c3h_run_frames at 8 frames per batch over 5 full
batches and a ragged one of 3, so every one of the four buffer sets is reused.  The frames
cycle over four resident grids made in numpy, shifted by one after four batches (a buffer
set's slot then holds another grid than the last time); the last frame is once `dense` and
once `tie`:

  dense   5 % random occupancy, random colours
  sparse  0.4 % random occupancy
  tie     a 4x4x4 block of random colours inside one subdivision: one non-empty feature row,
          so every box holding it, in every mode, sums that row and zeros and ties exactly;
          the record must be the first tied position in schedule, then scan order
  empty   no voxel

  case  grid     S  (D, M, r)      box                 rotate  reaches
  A     64^3     8  (20, 7, 12)    (1,2,3)             on      six modes, 2,016 positions, two model groups
  A'    64^3     8  (20, 7, 12)    (3,2,1), (2,3,1)    on      right after A: the same score layout (336
                                                               positions per mode), another gate pattern,
                                                               the sparse -1 fill over stale scores
  B     64^3     8  (20, 7, 12)    (2,2,1)             on      three modes
  C     64^3     8  (20, 7, 12)    (1,2,3)             off     one non-cubic mode
  D     64^3     8  (18, 3, 5)     (1,2,3)             on      D padded to 20, feature_max (the dense grid's
                                                               column maxima) in the tick's compress role,
                                                               one model group
  E     64x24x8  8  (20, 7, 12)    (1,2,3)             on      subdivisions (8,3,1): only modes 3 and 5
                                                               fit, so a mode's index is not its id
  E0    64x24x8  8  (20, 7, 12)    (1,2,3)             off     no position: the batch falls back to the lanes
  F     64^3     4  (100, 10, 20)  (1,2,3)             on      20,160 positions; dense: 20,157 pass (the
                                                               chunk loop), sparse: 303 (a ragged list)

Every case runs with score engines 1, 0 and 2.  Every frame went through the tick
(kernel_times; not E0); engines 0 and 2 give engine 1's records and last-frame scores() bit
for bit; the records are byte-identical with the pipeline off; against the oracle a record's
score is within 1e-5 relative of the oracle's at the record's own (mode, position), its mode
is the SearchMode id, its position the oracle's first maximum over the mode blocks in
schedule order unless tied within 2e-5; the tie frames are checked exactly; empty frames and
all of E0 give the cleared record; the last frame's scores() has the oracle's gated-out
pattern per mode block and is within 1e-5.

Streamed: case A through c3h_stream_frames in ragged pushes equals c3h_run_frames byte for
byte.  Points in: c3h_run_point_frames on a 64^3 canvas with clouds of three extents (the
canvas gate cuts other modes per frame) equals the single-frame path.  E0's single-frame
counterpart: a c3h_search none of whose modes fits applies the pending cleanMax (E0 found both
unwritten at rank 1).

The CPU test holds the conditions on the reference alone: several modes win with wide margins
(a tolerant position check cannot hide a wrong mode), the tie grids have one non-empty
subdivision, the pass counts above."""
import numpy as np
import pytest

import c3hlac
import pyoracle as po
from c3hlac import synth
from conftest import THR

RTOL = 1e-5
LEAF, F, EXIST = 0.04, 117, 10
BATCH, NFR = 8, 5 * 8 + 3
NAMES = ["dense", "sparse", "tie", "empty"]
CYCLES = {"dense": ["empty", "sparse", "tie", "dense"], "tie": ["sparse", "dense", "empty", "tie"]}
CUBE, FLAT = (64, 64, 64), (64, 24, 8)
CASES = {
    "A": dict(dims=CUBE, s=8, dmr=(20, 7, 12), box=(1, 2, 3), rotate=True, fmax=False),
    "B": dict(dims=CUBE, s=8, dmr=(20, 7, 12), box=(2, 2, 1), rotate=True, fmax=False),
    "C": dict(dims=CUBE, s=8, dmr=(20, 7, 12), box=(1, 2, 3), rotate=False, fmax=False),
    "D": dict(dims=CUBE, s=8, dmr=(18, 3, 5), box=(1, 2, 3), rotate=True, fmax=True),
    "E": dict(dims=FLAT, s=8, dmr=(20, 7, 12), box=(1, 2, 3), rotate=True, fmax=False),
    "E0": dict(dims=FLAT, s=8, dmr=(20, 7, 12), box=(1, 2, 3), rotate=False, fmax=False),
    "F": dict(dims=CUBE, s=4, dmr=(100, 10, 20), box=(1, 2, 3), rotate=True, fmax=False),
}
A_PRIME_BOXES = [(3, 2, 1), (2, 3, 1)]
# first cell of the tie block: inside one subdivision (at S = 4 it is that subdivision)
TIE_LO = {(CUBE, 8): (26, 26, 26), (CUBE, 4): (24, 24, 24), (FLAT, 8): (26, 10, 2)}
# the oracle's count of positions passing the gate, all modes together
NPASS = {"A": dict(dense=2016, sparse=1992), "E": dict(dense=19), "F": dict(dense=20157, sparse=303)}
# the oracle's record of the tie grid, (mode, x, y, z): the first tied position
TIE_FIRST = {"A": (0, 3, 2, 1), "B": (0, 2, 2, 3)}
TIE_COUNT = {"A": 36, "B": 12}  # tied positions over every mode


# ---------------------------------------------------------------- inputs and reference (CPU)
_WORDS, _FEATS, _REFS = {}, {}, {}


def _random_words(nvox, p):
    rng = np.random.default_rng(5)
    occ = rng.random(nvox) < p
    return np.where(occ, (1 << 24) | rng.integers(0, 1 << 24, nvox, dtype=np.uint32), 0).astype(np.uint32)


def _words(dims, s):
    """The four grids of one (grid, S): flat uint32 words in z, y, x order."""
    if (dims, s) not in _WORDS:
        gx, gy, gz = dims
        nvox = gx * gy * gz
        tie = np.zeros((gz, gy, gx), np.uint32)
        x0, y0, z0 = TIE_LO[dims, s]
        tie[z0:z0 + 4, y0:y0 + 4, x0:x0 + 4] = (1 << 24) | np.random.default_rng(7).integers(
            0, 1 << 24, (4, 4, 4), dtype=np.uint32)
        _WORDS[dims, s] = dict(dense=_random_words(nvox, 0.05), sparse=_random_words(nvox, 0.004),
                               tie=tie.reshape(-1), empty=np.zeros(nvox, np.uint32))
    return _WORDS[dims, s]


def _feats(dims, s):
    """The oracle's exact features, subdivisions and exist counts of the four grids."""
    if (dims, s) not in _FEATS:
        out = {}
        for k, w in _words(dims, s).items():
            g, layout, cloud = po.grid_inputs(w, dims, LEAF)
            fe, sb, _ = po.c3hlac(g, layout, cloud, F, THR, LEAF, s, exact=True)
            out[k] = (fe, sb, po.exist(fe))
        _FEATS[dims, s] = out
    return _FEATS[dims, s]


def _bases(dmr):
    return synth.random_bases(F, *dmr, seed=synth.BASE_SEED + 3)


def _fmax(case):
    if not case["fmax"]:
        return None
    fe = _feats(case["dims"], case["s"])["dense"][0]
    fm = np.maximum(fe.max(0), 1).astype(np.float32)
    assert fm.shape == (F,) and (fm > 1).any()
    return fm


def _blocks(sc, sb, box, rotate, M):
    """Splits the oracle's scores into the blocks of the modes that fit, in schedule order:
    [(SearchMode id, (xe, ye, ze), (M, P) scores in z, y, x scan order)]."""
    out, ofs = [], 0
    for mode, (xr, yr, zr) in zip(po.mode_schedule(box, rotate), po._mode_ranges(box, rotate)):
        xe, ye, ze = sb[0] - xr + 1, sb[1] - yr + 1, sb[2] - zr + 1
        if xe > 0 and ye > 0 and ze > 0:
            P = xe * ye * ze
            out.append((mode, (xe, ye, ze), sc[ofs:ofs + M * P].reshape(M, P)))
            ofs += M * P
    return out, ofs


def _first_max(blocks, m):
    """Model m's first maximum over the concatenated blocks (searchPart's strict '>' over the
    modes in schedule order): (block index, position, score), or None when nothing passes."""
    best = None
    for b, (_, _, sc) in enumerate(blocks):
        p = int(np.argmax(sc[m]))
        if sc[m, p] > 0 and (best is None or sc[m, p] > best[2]):
            best = (b, p, float(sc[m, p]))
    return best


def _ref(case, box=None):
    """The float64 oracle of the four grids for one case (and box): computed once."""
    box = case["box"] if box is None else box
    key = (case["dims"], case["s"], case["dmr"], box, case["rotate"], case["fmax"])
    if key not in _REFS:
        axis_t, var, axis_q = _bases(case["dmr"])
        ap = synth.whiten(axis_t, var)
        M = case["dmr"][1]
        ref = {}
        for k, (fe, sb, ex) in _feats(case["dims"], case["s"]).items():
            L, _, sc = po.search(sb, fe, ex, ap, axis_q, box, 1, EXIST, rotate=case["rotate"], dbl=True,
                                 fmax=_fmax(case), want_scores=True)
            blocks, total = _blocks(sc, sb, box, case["rotate"], M)
            assert total == (sc.size if total else 0)
            # the oracle's own record is the first maximum over the concatenated blocks
            for m, ((s, x, y, z, mode),) in enumerate(L.records()):
                fm = _first_max(blocks, m)
                if fm is None:
                    assert (s, x, y, z, mode) == (0.0, 0, 0, 0, 0)
                else:
                    md, (xe, ye, _), _ = blocks[fm[0]]
                    assert (s, mode, (z * ye + y) * xe + x) == (fm[2], md, fm[1]), (key, k, m)
            ref[k] = dict(blocks=blocks, total=total, records=[r[0] for r in L.records()])
        _REFS[key] = ref
    return _REFS[key]


def _frame_name(i, cycle):
    return cycle[(i + i // (4 * BATCH)) % 4]  # shifted by one once every buffer set was used


def _names(last):
    names = [_frame_name(i, CYCLES[last]) for i in range(NFR)]
    assert names[-1] == last and set(names[:BATCH]) == set(NAMES)
    assert any(names[i] != names[i + 4 * BATCH] for i in range(NFR - 4 * BATCH))  # a set's slot changes grid
    return names


def test_reference_conditions():
    """Conditions on the inputs and the oracle alone (no GPU)."""
    for key in ("A", "B", "D", "E", "F"):
        case = CASES[key]
        M = case["dmr"][1]
        ref = _ref(case)
        sched = po.mode_schedule(case["box"], True)
        winners = []
        for k in ("dense", "sparse"):
            blocks = ref[k]["blocks"]
            ids = [b[0] for b in blocks]
            assert ids == ([3, 5] if key == "E" else sched), (key, ids)
            best = np.stack([b[2].max(1) for b in blocks])  # (modes, M)
            assert (best > 0).all(), (key, k)
            win = best.argmax(0)
            winners += [ids[i] for i in win]
            assert [r[4] for r in ref[k]["records"]] == [ids[i] for i in win], (key, k)
            # the winning mode leads every other mode by more than 1e-3 relative (50 x the tie
            # tolerance) in at least two thirds of the models
            srt = np.sort(best, 0)
            wide = int(((srt[-1] - srt[-2]) > 1e-3 * srt[-1]).sum())
            assert 3 * wide >= 2 * M, (key, k, wide, M)
            if k in NPASS.get(key, {}):
                assert sum(int((b[2][0] >= 0).sum()) for b in blocks) == NPASS[key][k], (key, k)
        if key == "E":
            assert set(winners) == {3, 5}
        else:
            assert len(set(winners)) >= (2 if key == "B" else 3) and any(w != 0 for w in winners), (key, winners)
        # the tie grid: one non-empty subdivision, every position holding it ties exactly, and
        # the oracle's record is the first of them
        fe, sb, ex = _feats(case["dims"], case["s"])["tie"]
        assert np.count_nonzero(ex) == 1 and np.count_nonzero(fe.any(1)) == 1 and ex.max() > EXIST, key
        blocks = ref["tie"]["blocks"]
        for m in range(M):
            pos = np.concatenate([b[2][m] for b in blocks])
            assert np.unique(pos[pos > 0]).size == 1, (key, m)
            if key in TIE_COUNT:
                assert int((pos > 0).sum()) == TIE_COUNT[key], (key, m)
            b, p, s = _first_max(blocks, m)
            assert p == int(np.flatnonzero(blocks[b][2][m] > 0)[0]) and not any((x[2][m] > 0).any() for x in blocks[:b])
            s_, x, y, z, mode = ref["tie"]["records"][m]
            if key in TIE_FIRST:
                assert (mode, x, y, z) == TIE_FIRST[key], (key, m)
            if key == "E":
                assert (mode, x, y, z) == (3, 2, 0, 0), m
        assert all(not b[2].size or (b[2] == -1).all() for b in ref["empty"]["blocks"])
    # A': the same score layout as A, another gate pattern on the grids that gate anything out
    boxes = [CASES["A"]["box"]] + A_PRIME_BOXES
    for b in boxes:
        assert [blk[2].shape for blk in _ref(CASES["A"], b)["dense"]["blocks"]] == [(7, 336)] * 6
    for k in ("sparse", "tie"):
        gate = [np.concatenate([blk[2][0] < 0 for blk in _ref(CASES["A"], b)[k]["blocks"]]) for b in boxes]
        assert gate[0].any() and not np.array_equal(gate[0], gate[1]) and not np.array_equal(gate[1], gate[2]), k
    assert _ref(CASES["E"])["dense"]["total"] == 19 * 7 and _ref(CASES["F"])["dense"]["total"] == 20160 * 10
    assert _ref(CASES["E0"])["dense"]["blocks"] == [] and len(_ref(CASES["C"])["dense"]["blocks"]) == 1
    for last in CYCLES:
        _names(last)


# ---------------------------------------------------------------- the GPU runs
@pytest.fixture(scope="module")
def grids(ctx):
    """Device copies of the resident grids, per (grid, S)."""
    import torch
    out = {}
    for key in sorted({(c["dims"], c["s"]) for c in CASES.values()}):
        out[key] = {k: torch.from_numpy(w.view(np.int32)).to("cuda:0") for k, w in _words(*key).items()}
    torch.cuda.synchronize()
    return out


def _setup(ctx, case):
    ctx.search_setup(*_bases(case["dmr"]), feature_max=_fmax(case))
    ctx.set_rank(1)
    ctx.set_batch(BATCH)
    ctx.set_pipeline(True)


def _restore(ctx):
    ctx.timing(False)
    ctx.set_score_engine(0)
    ctx.set_batch(32)
    ctx.set_pipeline(True)


def _run_frames(ctx, grids, case, box, names, pushes=None):
    """One c3h_run_frames (pushes: c3h_stream_frames in pieces and a flush) over the frame
    sequence: (NFR, M, 3) int64 record words, frames counted by the tick's timer."""
    import torch
    M = case["dmr"][1]
    d_words = grids[case["dims"], case["s"]]
    ptrs = np.array([d_words[k].data_ptr() for k in names], np.uint64)
    d_out = torch.full((NFR, M * 3), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.timing(c3hlac.timing_mask("pipeline"))
    ctx.kernel_times(reset=True)
    args = (case["dims"], (0, 0, 0), LEAF, F, THR, case["s"], box, EXIST, case["rotate"])
    if pushes is None:
        ctx.run_frames(ptrs, *args, d_out.data_ptr())
    else:
        f0 = 0
        for n in pushes:
            ctx.run_frames(ptrs[f0:f0 + n], *args, d_out[f0:].data_ptr(), stream=True)
            f0 += n
        assert f0 == NFR
        ctx.stream_flush()
    ctx.synchronize()
    kt = ctx.kernel_times(reset=True)
    ctx.timing(False)
    return d_out.cpu().numpy().reshape(NFR, M, 3), kt["pipeline"][1]


def _run_engines(ctx, grids, case, box, names, through_tick=True):
    """The pipelined run with engines 1, 0 and 2: records and last-frame scores per engine."""
    got, scores = {}, {}
    for engine in (1, 0, 2):
        ctx.set_score_engine(engine)
        got[engine], ticked = _run_frames(ctx, grids, case, box, names)
        if through_tick:
            assert ticked == NFR, ("frames through the tick", engine, ticked)
        scores[engine] = ctx.scores()
    ctx.set_score_engine(0)
    return got, scores


def _run_lanes(ctx, grids, case, box, names):
    ctx.set_pipeline(False)
    try:
        return _run_frames(ctx, grids, case, box, names)[0]
    finally:
        ctx.set_pipeline(True)


def _decode(rec_m):
    s = float(rec_m[0:1].view(np.float64)[0])
    x, y, z, mode = (int(v) for v in rec_m[1:3].view(np.int32))
    return s, x, y, z, mode


def _check_det(rec, ref_k, tag, exact):
    """rec: (M, 3) int64 c3h_det words of one frame against the oracle's mode blocks."""
    blocks = ref_k["blocks"]
    for m in range(rec.shape[0]):
        s, x, y, z, mode = _decode(rec[m])
        fm = _first_max(blocks, m)
        if fm is None:  # nothing passes the gate (or no mode fits): the cleared record
            assert (s, x, y, z, mode) == (0.0, 0, 0, 0, 0), (tag, m, (s, x, y, z, mode))
            continue
        ids = [b[0] for b in blocks]
        assert mode in ids, (tag, m, "mode", mode, "fitting modes", ids)
        _, (xe, ye, ze), sc = blocks[ids.index(mode)]
        assert 0 <= x < xe and 0 <= y < ye and 0 <= z < ze, (tag, m, mode, (x, y, z), (xe, ye, ze))
        p = (z * ye + y) * xe + x
        assert sc[m, p] > 0 and abs(s - sc[m, p]) <= RTOL * sc[m, p], (tag, m, mode, (x, y, z), s, sc[m, p])
        bmode, bp, bs = ids[fm[0]], fm[1], fm[2]
        if exact:
            assert (mode, p) == (bmode, bp), (tag, m, (mode, x, y, z), ref_k["records"][m])
        elif (mode, p) != (bmode, bp):  # only a tie within tolerance may pick another position
            assert sc[m, p] >= bs * (1 - 2 * RTOL), (tag, m, (mode, x, y, z), ref_k["records"][m])


def _check_run(got, scores, lanes, ref, names, tag):
    """Checks 2 to 6 of one pipelined run (all engines) against the lanes and the oracle."""
    last = names[-1]
    M = got[1].shape[1]
    for engine in (0, 2):  # engines agree bit for bit: every record, the last frame's scores
        bad = np.flatnonzero((got[engine] != got[1]).any(axis=(1, 2)))
        assert bad.size == 0, (tag, "records", engine, bad[:8].tolist(), [names[i] for i in bad[:8]])
        assert np.array_equal(scores[engine], scores[1]), (tag, "scores", engine)
    bad = [i for i in range(NFR) if got[1][i].tobytes() != lanes[i].tobytes()]
    assert not bad, (tag, "pipeline != lanes", len(bad), bad[:8], [names[i] for i in bad[:8]])
    gs = scores[1]
    assert gs.size == ref[last]["total"], (tag, gs.size, ref[last]["total"])
    if last == "tie" and gs.size:  # the tied scores are bit-identical: one row plus zeros
        ofs, per_model = 0, [[] for _ in range(M)]
        for _, _, sc in ref[last]["blocks"]:
            blk = gs[ofs:ofs + sc.size].reshape(sc.shape)
            ofs += sc.size
            for m in range(M):
                per_model[m].append(blk[m])
        for m in range(M):
            v = np.concatenate(per_model[m])
            o = np.concatenate([b[2][m] for b in ref[last]["blocks"]])
            assert np.unique(v[v > 0]).size == 1 and int((v > 0).sum()) == int((o > 0).sum()), (tag, "tied scores", m)
    for i, k in enumerate(names):
        _check_det(got[1][i], ref[k], "%s frame %d (%s)" % (tag, i, k), exact=(k == "tie"))
    ofs = 0
    for mode, _, sc in ref[last]["blocks"]:  # the last frame's scores, per mode block
        blk = gs[ofs:ofs + sc.size].reshape(sc.shape)
        ofs += sc.size
        assert np.array_equal(blk < 0, sc < 0), (tag, "gated-out positions of mode", mode)
        assert ((blk < 0) <= (blk == -1)).all()
        ok = sc > 0
        np.testing.assert_allclose(blk[ok], sc[ok], rtol=RTOL, err_msg="%s mode %d" % (tag, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("last", ["dense", "tie"])
@pytest.mark.parametrize("key", list(CASES))
def test_tick_modes_engines_lanes_and_oracle(ctx, grids, key, last):
    case, names = CASES[key], _names(last)
    ref = _ref(case)
    _setup(ctx, case)
    try:
        got, scores = _run_engines(ctx, grids, case, case["box"], names, through_tick=(key != "E0"))
        lanes = _run_lanes(ctx, grids, case, case["box"], names)
    finally:
        _restore(ctx)
    if key == "E0":  # no mode fits: every frame's record is the setRank state
        assert ref[last]["total"] == 0
        for engine in (1, 0, 2):
            assert not got[engine].any(), (key, engine)
        assert not lanes.any()
    _check_run(got, scores, lanes, ref, names, "%s last=%s" % (key, last))


@pytest.mark.gpu
@pytest.mark.parametrize("rank", [1, 2])
def test_single_frame_search_without_a_fitting_mode_applies_clean_max(ctx, rank):
    """E0 on the single-frame path: a search none of whose modes fits finds no candidate, but
    the lists it hands out have taken the pending cleanMax (scores and positions zeroed, modes
    kept: search.cpp:683-690), at rank 1 as at rank 2."""
    case = CASES["E"]
    M = case["dmr"][1]
    ctx.search_setup(*_bases(case["dmr"]))
    ctx.set_grid(_words(case["dims"], case["s"])["dense"], case["dims"], (0, 0, 0), LEAF)
    ctx.extract(F, THR, case["s"])
    try:
        ctx.set_rank(rank)
        first, nm = ctx.search(case["box"], EXIST)
        first = first.copy()
        assert nm == 6 and (first["score"][:, 0] > 0).all() and set(first["mode"][:, 0].tolist()) <= {3, 5}
        ctx.clean_max()
        held, _ = ctx.search(case["box"], EXIST, rotate=False)
        want = np.zeros((M, rank), c3hlac.DET_DTYPE)
        want["mode"] = first["mode"]
        assert np.array_equal(held, want), (held, want)
        assert ctx.scores().size == 0
    finally:
        ctx.set_rank(1)


@pytest.mark.gpu
@pytest.mark.parametrize("last", ["dense", "tie"])
def test_other_boxes_of_the_same_layout_right_after_case_a(ctx, grids, last):
    """A': boxes (3,2,1) and (2,3,1) keep A's score layout (six blocks of 336 positions), so
    the gate's sparse -1 fill runs over the scores of another box."""
    case, names = CASES["A"], _names(last)
    boxes = [case["box"]] + A_PRIME_BOXES
    refs = {b: _ref(case, b) for b in boxes}
    _setup(ctx, case)
    runs, lanes = {}, {}
    try:
        for b in boxes:  # back to back: nothing else touches the context's scores in between
            runs[b] = _run_engines(ctx, grids, case, b, names)
        for b in boxes:
            lanes[b] = _run_lanes(ctx, grids, case, b, names)
    finally:
        _restore(ctx)
    for b in boxes:
        _check_run(runs[b][0], runs[b][1], lanes[b], refs[b], names, "A' box %s last=%s" % (b, last))


@pytest.mark.gpu
def test_streamed_case_a_equals_run_frames(ctx, grids):
    """Case A through c3h_stream_frames in ragged pushes and a flush: c3h_run_frames' records."""
    case, names = CASES["A"], _names("dense")
    _setup(ctx, case)
    try:
        whole, ticked = _run_frames(ctx, grids, case, case["box"], names)
        assert ticked == NFR
        streamed, ticked = _run_frames(ctx, grids, case, case["box"], names, pushes=[8, 24, 5, 6])
        assert ticked == NFR
    finally:
        _restore(ctx)
    assert (whole[:, :, 0].view(np.float64)[[i for i, k in enumerate(names) if k != "empty"]] > 0).all()
    bad = [i for i in range(NFR) if streamed[i].tobytes() != whole[i].tobytes()]
    assert not bad, (len(bad), bad[:8], [names[i] for i in bad[:8]])


P_G, P_LEAF, P_S, P_DMR, P_BATCH, P_NFR = 64, 0.02, 8, (20, 3, 12), 4, 12
P_BOXES = [(2, 2, 1), (1, 2, 3)]
P_EXTENTS = [(64, 40, 16), (16, 64, 40), (40, 16, 64)]  # subdivisions (8,5,2), (2,8,5), (5,2,8)


@pytest.mark.gpu
def test_point_frames_with_clouds_of_three_extents(ctx):
    """c3h_run_point_frames at rank 1 on a 64^3 canvas: the canvas gate bounds every frame's
    positions by the frame's own subdivisions, which cuts other modes per extent; every frame
    stays in its batch (status 0) with the single-frame path's records."""
    import torch
    frames = []
    for i in range(P_NFR):
        ex, ey, ez = P_EXTENTS[i % 3]
        rng = np.random.default_rng(100 + i)
        nv = ex * ey * ez
        idx = np.unique(np.concatenate([rng.choice(nv, nv // 20, replace=False), [0, nv - 1]]))
        xyz = np.stack([idx % ex, idx // ex % ey, idx // (ex * ey)], 1)
        pts = np.empty((idx.size, 4), np.float32)
        pts[:, :3] = ((xyz + 0.5) * P_LEAF).astype(np.float32)  # voxel centres
        pts[:, 3] = rng.integers(0, 1 << 24, idx.size, dtype=np.uint32).view(np.float32)
        frames.append(pts)
    M = P_DMR[1]
    ctx.search_setup(*_bases(P_DMR))
    ctx.set_rank(1)
    ctx.set_batch(P_BATCH)
    ctx.set_pipeline(True)
    got, single = {}, {}
    try:
        for box in P_BOXES:
            d_out = torch.full((P_NFR, M * 3), -1, dtype=torch.int64, device="cuda:0")
            nm, info = ctx.run_point_frames(frames, P_LEAF, (P_G,) * 3, F, THR, P_S, box, EXIST, True, d_out)
            assert nm == len(po.mode_schedule(box))
            assert (info["status"] == 0).all(), (box, info["status"])
            for i in range(P_NFR):
                assert tuple(info["div_b"][i]) == P_EXTENTS[i % 3], (i, info["div_b"][i])
                assert tuple(info["subdiv_b"][i]) == tuple(e // P_S for e in P_EXTENTS[i % 3]), (i, info["subdiv_b"][i])
            got[box] = d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(P_NFR, M)
            ref = []
            for i in range(P_NFR):
                ctx.voxelize(frames[i], P_LEAF)
                ctx.extract(F, THR, P_S)
                ctx.set_rank(1)
                lists, _ = ctx.search(box, EXIST)
                ref.append(lists[:, 0].copy())
            single[box] = ref
    finally:
        ctx.set_batch(32)
    for box in P_BOXES:
        ranges = dict(zip(po.mode_schedule(box), po._mode_ranges(box, True)))
        modes = set()
        for i in range(P_NFR):
            assert np.array_equal(got[box][i], single[box][i]), (box, i, got[box][i], single[box][i])
            assert (got[box][i]["score"] > 0).all(), (box, i)
            sb = tuple(e // P_S for e in P_EXTENTS[i % 3])
            for rec in got[box][i]:  # the record's box lies inside the frame's own subdivisions
                rr = ranges[int(rec["mode"])]
                assert all(int(rec[a]) + rr[j] <= sb[j] for j, a in enumerate("xyz")), (box, i, rec, sb)
                modes.add(int(rec["mode"]))
        assert len(modes) >= 2 and modes != {0}, (box, modes)
