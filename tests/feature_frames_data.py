"""Frames of caller-computed feature rows shared by test_feature_frames_cpu.py and
test_gpu_feature_frames.py, on the (16, 16, 16) subdivision canvas of batch_grids at S = 4.

VOSCH-shaped frames (dim 137, rule VOSCH): a row is [g | C3-HLAC-117 row of batch_grids], g =
20 columns of floor(random * 40) kept on the rows whose C3 part is non-zero and on 20 % of the
others, so the VOSCH rule (f20, f21 = the C3 part's first two bins) equals the C3 exist and
the kept 20 % are rows with data and exist 0 -- rows the search must add although the gate
counts nothing for them.  feature_max = 0.9 x the column maximum, entry 5 = 0.

GRSD-shaped frames (dim 21, rule GRSD): test_gpu_set_features.py's construction with
default_rng(8) and half the rows zeroed: rows of few transitions have exist 0 and data.

Cropped frames: the x < 13, y < 16, z < 9 block of a VOSCH frame re-laid in its own counts,
and the x < 1 slab (1, 16, 16), which no 2x2x2 box fits.

Oracle results are computed once per (kind, case) and shared."""
import numpy as np

import batch_grids as bg
import pyoracle as po
from c3hlac import synth

S = 4
CANVAS = (16, 16, 16)
H = 16 ** 3
CROP = (13, 16, 9)
SLAB = (1, 16, 16)

# (rule, dim, D, M, r, box, exist threshold, rotate, rank)
VOSCH = dict(rule=1, dim=137, D=100, M=3, r=20, thr=bg.EXIST)
GRSD = dict(rule=2, dim=21, D=20, M=2, r=5, thr=60)
WIDE = dict(rule=1, dim=137, D=100, M=3, r=70, thr=bg.EXIST)

_FR, _SETUP, _ORACLE = {}, {}, {}


def vosch_exist(f):
    """search_new.h:41-43 in numpy (test_gpu_set_features.py)."""
    t = (f[:, 20] + f[:, 21]).astype(np.float32) * np.float32(2)
    return (t.astype(np.float64) + 0.001).astype(np.int32)


def grsd_exist(f):
    """search_new.h:69-74 in numpy."""
    e = np.zeros(f.shape[0], np.int32)
    for i in range(20):
        e = (e.astype(np.float32) + f[:, i]).astype(np.int32)
    return e // 26


def crop(f, counts, src=CANVAS):
    """The x < counts[0], y < counts[1], z < counts[2] block of a frame laid out in `src`
    counts, re-laid in its own counts (row h = x + y * xn + z * xn * yn)."""
    v = f.reshape(src[2], src[1], src[0], f.shape[1])
    return np.ascontiguousarray(v[:counts[2], :counts[1], :counts[0]]).reshape(-1, f.shape[1])


def vosch_frame(name):
    """-> (rows (4096, 137) float32, exist) of kind dense / sparse / empty."""
    if ("vosch", name) not in _FR:
        fe, sb, ex = bg.feats(S, name)
        assert tuple(int(v) for v in sb) == CANVAS
        rng = np.random.default_rng(11)
        g = np.floor(rng.random((H, 20)) * 40).astype(np.float32)
        keep = fe.any(1) | (rng.random(H) < 0.2)
        g[~keep] = 0
        f = np.ascontiguousarray(np.concatenate([g, fe.astype(np.float32)], 1))
        e = vosch_exist(f)
        assert np.array_equal(e, ex), "the VOSCH rule equals the C3 exist of the rows' C3 part"
        _FR["vosch", name] = (f, e)
    return _FR["vosch", name]


def grsd_frame(name):
    """-> (rows (4096, 21) float32, exist): dense = the construction above, sparse = another
    40 % of the rows zeroed, empty = no data."""
    if ("grsd", name) not in _FR:
        rng = np.random.default_rng(8)
        f = np.floor(rng.random((H, 21)) * 60).astype(np.float32)
        few = rng.random(H) < 0.25
        f[few] = np.floor(rng.random((few.sum(), 21)) * 2)
        f[rng.random(H) < 0.5] = 0
        if name == "sparse":
            f[rng.random(H) < 0.4] = 0
        if name == "empty":
            f[:] = 0
        _FR["grsd", name] = (f, grsd_exist(f))
    return _FR["grsd", name]


def frame(kind, name):
    """kind: 'vosch', 'grsd', 'crop' (13, 16, 9) or 'slab' (1, 16, 16) -> (rows, exist, counts)."""
    if kind == "vosch":
        return vosch_frame(name) + (CANVAS,)
    if kind == "grsd":
        return grsd_frame(name) + (CANVAS,)
    counts = CROP if kind == "crop" else SLAB
    if (kind, name) not in _FR:
        f, e = vosch_frame(name)
        _FR[kind, name] = (crop(f, counts), crop(e[:, None], counts)[:, 0].copy())
    return _FR[kind, name] + (counts,)


def data_rows_without_exist(kind, name):
    f, e, _ = frame(kind, name)
    return f.any(1) & (e == 0)


def setup(case):
    """-> (axis_t, var, axis_q, feature_max) of a case (VOSCH / GRSD / WIDE)."""
    key = (case["dim"], case["D"], case["M"], case["r"])
    if key not in _SETUP:
        dim, D, M, r = key
        if r <= D:
            axis_t, var, axis_q = synth.random_bases(dim, D, M, r, seed=synth.BASE_SEED + 15)
        else:  # more rows than dimensions: any M x r x D (batch_grids.bases)
            axis_t, var, _ = synth.random_bases(dim, D, 1, D, seed=synth.BASE_SEED + 15)
            axis_q = (np.random.default_rng(2).standard_normal((M, r, D)) / np.sqrt(r)).astype(np.float32)
        fmax = None
        if case["rule"] == 1:
            cols = np.max([vosch_frame(k)[0].max(0) for k in bg.NAMES], 0)
            fmax = (cols * np.float32(0.9)).astype(np.float32)
            fmax[5] = 0
        _SETUP[key] = (axis_t, var, axis_q, fmax)
    return _SETUP[key]


def oracle(case, kind, name, box, rank=1, rotate=True, zero_hidden=False):
    """-> (Lists, scores (float64, c3h_get_scores layout of the frame's own counts)).
    zero_hidden: the rows with data and exist 0 zeroed first (what a search that skipped rows
    by their exist value would compute)."""
    key = (case["dim"], case["D"], case["M"], case["r"], kind, name, tuple(box), rank, rotate, zero_hidden)
    if key not in _ORACLE:
        f, e, counts = frame(kind, name)
        if zero_hidden:
            f = f.copy()
            f[data_rows_without_exist(kind, name)] = 0
        axis_t, var, axis_q, fmax = setup(case)
        L, _, sc = po.search(counts, f, e, synth.whiten(axis_t, var), axis_q, box, rank, case["thr"], rotate=rotate,
                             dbl=True, fmax=fmax, want_scores=True)
        _ORACLE[key] = (L, sc)
    return _ORACLE[key]


def canvas_to_frame_scores(sc, M, counts, box, canvas=CANVAS):
    """Scores of one mode (box as given, no rotation) in the canvas layout -> (inside, outside):
    the (M, ze, ye, xe) block of the positions inside the frame's own counts, and the rest."""
    ce = [c - b + 1 for c, b in zip(canvas, box)]
    fe = [max(c - b + 1, 0) for c, b in zip(counts, box)]
    v = sc.reshape(M, ce[2], ce[1], ce[0])
    inside = v[:, :fe[2], :fe[1], :fe[0]]
    mask = np.ones(v.shape, bool)
    mask[:, :fe[2], :fe[1], :fe[0]] = False
    return inside, v[mask]
