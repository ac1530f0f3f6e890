"""Grids and oracle references shared by test_gpu_tick_wide.py and
test_gpu_remove_overlap_batch.py: 64^3 grids built on the CPU from packed words, the oracle's
exact C3-HLAC-117 features per (S, grid) and its float64 scores per (models, S, box, grid),
each computed once per session.

  dense   5 % random occupancy, random colours (default_rng(5)): every position passes
  sparse  a one-voxel-thick wavy surface, colours from default_rng(6): a depth camera's view
  empty   no voxel: nothing passes
"""
import numpy as np

import pyoracle as po
from c3hlac import synth
from conftest import THR

G, LEAF, F, EXIST = 64, 0.04, 117, 10
BATCH, NFR = 8, 5 * 8 + 3
NAMES = ["dense", "sparse", "empty"]

_WORDS, _FEATS, _BASES, _SCORES = {}, {}, {}, {}


def words():
    if not _WORDS:
        rng = np.random.default_rng(5)
        occ = rng.random(G ** 3) < 0.05
        _WORDS["dense"] = np.where(occ, (1 << 24) | rng.integers(0, 1 << 24, G ** 3, dtype=np.uint32),
                                   0).astype(np.uint32)
        rng = np.random.default_rng(6)
        y, x = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
        z = np.rint(30 + 9 * np.sin(x / 9.0) + 7 * np.cos(y / 7.0)).astype(np.int64)
        surf = np.zeros((G, G, G), np.uint32)  # [z][y][x]
        surf[z, y, x] = (1 << 24) | rng.integers(0, 1 << 24, (G, G), dtype=np.uint32)
        _WORDS["sparse"] = surf.reshape(-1)
        _WORDS["empty"] = np.zeros(G ** 3, np.uint32)
    return _WORDS


def feats(s, name):
    """-> (features, subdivisions, exist) of the oracle's exact extract."""
    if (s, name) not in _FEATS:
        g, layout, cloud = po.grid_inputs(words()[name], (G,) * 3, LEAF)
        fe, sb, _ = po.c3hlac(g, layout, cloud, F, THR, LEAF, s, exact=True)
        _FEATS[s, name] = (fe, sb, po.exist(fe))
    return _FEATS[s, name]


def bases(D, M, r):
    if (D, M, r) not in _BASES:
        if r <= D:
            _BASES[D, M, r] = synth.random_bases(F, D, M, r, seed=synth.BASE_SEED + 3)
        else:  # more rows than dimensions: no orthonormal set, the API takes any M x r x D
            # (seed 2: the top scores of (20, 2, 70) are clear of each other, test_gpu_tick_wide.py)
            axis_t, var, _ = synth.random_bases(F, D, 1, D, seed=synth.BASE_SEED + 3)
            rng = np.random.default_rng(2)
            axis_q = (rng.standard_normal((M, r, D)) / np.sqrt(r)).astype(np.float32)
            _BASES[D, M, r] = (axis_t, var, axis_q)
    return _BASES[D, M, r]


def oracle_search(D, M, r, s, box, name, rank=1, rotate=True):
    """-> (Lists, scores (float64, c3h_get_scores layout), subdivisions) of the float64 oracle."""
    key = (D, M, r, s, tuple(box), name, rank, rotate)
    if key not in _SCORES:
        axis_t, var, axis_q = bases(D, M, r)
        fe, sb, ex = feats(s, name)
        L, _, sc = po.search(sb, fe, ex, synth.whiten(axis_t, var), axis_q, box, rank, EXIST, rotate=rotate, dbl=True,
                             want_scores=True)
        _SCORES[key] = (L, sc, sb)
    return _SCORES[key]


def frame_names(last):
    """The frame cycle over the three grids, shifted after every fourth batch (once each of the
    four buffer sets was used), so a set's slot holds another grid than the time before."""
    k = NAMES.index(last)
    cycle = [NAMES[(k + 1 + j) % 3] for j in range(3)]
    shift = (NFR - 1 + 2 * ((NFR - 1) // (4 * BATCH))) % 3
    names = [cycle[(i + 2 * (i // (4 * BATCH)) - shift + 2 + 3) % 3] for i in range(NFR)]
    assert names[-1] == last and set(names[:BATCH]) == set(NAMES)
    assert any(names[i] != names[i + 4 * BATCH] for i in range(NFR - 4 * BATCH))
    return names


def lists_records(L):
    """oracle Lists -> (M, rank) structured array in c3hlac.DET_DTYPE."""
    import c3hlac
    out = np.zeros(L.M * L.rank, c3hlac.DET_DTYPE)
    out["score"], out["x"], out["y"], out["z"], out["mode"] = L.score, L.x, L.y, L.z, L.mode
    return out.reshape(L.M, L.rank)
