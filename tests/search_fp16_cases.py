"""Inputs shared by test_search_fp16_ref_cpu.py and test_gpu_search_fp16.py: the (D, M, r)
shape table of the f16 projection kernels, synthetic feature rows and the bases.

Rows: F = 117 features for D <= 116, else 981; half of the entries zero, the rest uniform
in [0, 1), so box rows point in different directions; about 30 % of the rows all zero with
exist 0, the others exist 1..9.  Each z plane carries a power of two from Z_EXP:
box rows span 2^-22 .. 2^20, beyond float16's range at both ends, so the kernels' power-of-
two scale is load-bearing (without it rows overflow to inf or sink into the subnormals).
The scene axis is synth.random_bases', the models are np_ref.flat_bases'."""
import numpy as np

import np_ref as npr
from c3hlac import synth

SB = (13, 11, 9)
# (D, M, r): kernel, edge
TABLE = [
    (100, 5, 70),   # f16s: the production r; rp = 72; KQ = 7 with a 4-wide k tail
    (16, 4, 16),    # f16s: KQ = 1; two model ends per tile, one exactly at the tile's end
    (16, 1, 16),    # f16s: half-empty last tile: a phantom model boundary past the group
    (128, 3, 17),   # f16s: rp = 20 zero-padded columns; ends at 20, 40, 60; KQ = 8
    (36, 2, 33),    # f16s: odd tile count (accumulator alternation tail); D % 16 = 4
    (160, 9, 64),   # f16s: KQ = 10; ss_groups -> 2 uneven groups (4 + 5 models); D > 128
    (12, 3, 5),     # f16: D < 16 (clamped k); one partial tile
    (40, 7, 3),     # f16: 21 columns; small scores
    (100, 10, 13),  # f16: 130 columns; models straddling four tile edges; the group count
    (4, 1, 1),      # f16: the smallest everything
]
Z_EXP = (-22, -18, -18, 0, 18, 18, 20, 20, 20)


def feature_dim(D):
    return 117 if D <= 116 else 981


# r = 1 scores are a single |cos|: rows of free direction bring it arbitrarily close to 0,
# where the absolute error of any f32 accumulation (~1e-8) is no longer small relative to
# the score.  These shapes' rows share a component (COMMON x one random row), which keeps
# every score away from 0 (test_search_fp16_ref_cpu.py asserts >= 0.01 for every shape).
COMMON = {(4, 1, 1): 2.0}


def rows(D, seed, sb=SB, zero_frac=0.3, common=0.0, z_exp=True):
    """-> feat (H, F) float32, exist (H,) int32.  z_exp=False: no powers of two (rows the
    f16 compress accepts: its operands are not scaled)."""
    xn, yn, zn = sb
    H, F = xn * yn * zn, feature_dim(D)
    rng = np.random.default_rng(seed)
    feat = rng.random((H, F), dtype=np.float32) * (rng.random((H, F)) < 0.5)
    feat = feat + np.float32(common) * rng.random(F, dtype=np.float32)[None, :]
    z = np.arange(H) // (xn * yn)
    e = np.asarray(Z_EXP)[z * len(Z_EXP) // zn]
    if z_exp:
        feat = np.ldexp(feat, e[:, None]).astype(np.float32)
    exist = rng.integers(1, 10, H).astype(np.int32)
    zero = rng.random(H) < zero_frac
    feat[zero] = 0
    exist[zero] = 0
    return feat, exist


def inputs(shape, sb=SB):
    """The table shape's inputs -> feat, exist, axis_t, var, axis_q."""
    D, M, r = shape
    seed = 1000 * D + 10 * M + r
    feat, exist = rows(D, seed, sb, common=COMMON.get(shape, 0.0))
    return (feat, exist) + bases(D, M, r, seed)


def exact_rows(D, seed, count, sb=SB):
    """Rows and thr for which exactly `count` (1, 33 or 0) positions of box (2, 2, 2) pass:
    exist is 0 / 1 and thr = 7, so a position passes iff all 8 cells of its box exist (thr = 8
    for count 0: none can).  -> feat, exist, thr."""
    xn, yn, zn = sb
    feat, _ = rows(D, seed, sb, zero_frac=0.0)
    ev = np.zeros((zn, yn, xn), np.int32)
    if count == 1:
        ev[4:6, 5:7, 6:8] = 1
    else:  # three bars of 12 x 2 x 2 cells: 11 positions each
        for y0 in (0, 3, 6):
            ev[3:5, y0:y0 + 2, 0:12] = 1
    exist = ev.reshape(-1)
    feat[exist == 0] = 0
    return feat, exist, (8 if count == 0 else 7)


def bases(D, M, r, seed):
    """-> axis_t (D, F), var (D,), axis_q (M, r, D)."""
    axis_t, var, _ = synth.random_bases(feature_dim(D), D, 1, 1, seed=seed)
    return axis_t, var, npr.flat_bases(D, M, r, seed + 1)


def median_thr(exist, sb, ranges):
    """The median exist count of mode 0's boxes: just under half of the positions pass."""
    xn, yn, zn = sb
    eb = npr.box_sums(np.asarray(exist, np.int64).reshape(zn, yn, xn), *ranges)
    return int(np.median(eb))


def compress_f32(feat, axis_t, var):
    """A float32 G for the CPU tests (the GPU tests take Context.compressed())."""
    return (feat.astype(np.float64) @ synth.whiten(axis_t, var).T.astype(np.float64)).astype(np.float32)


def flat(mode_scores):
    """scores() / scores_f16() output in Context.scores()' flat (mode, M, P) layout."""
    return np.concatenate([sc.reshape(-1) for _, _, _, sc in mode_scores]) if mode_scores else np.zeros(0)


def contract_excess(s, ref64):
    """The published fp16 contract: |s - ref| <= max(RTOL * ref, ATOL) on passing scores.
    -> the largest |s - ref| / max(RTOL * ref, ATOL) (<= 1 when the contract holds)."""
    lim = np.maximum(npr.F16_CONTRACT_RTOL * ref64, npr.F16_CONTRACT_ATOL)
    return float((np.abs(s - ref64) / lim).max()) if s.size else 0.0
