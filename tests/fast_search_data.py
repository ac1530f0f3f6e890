"""Cases and references for the fp32 fast search route (compressed dimension D <= 160):
test_fast_search_data_cpu.py checks the inputs and the references against each other,
test_gpu_fast_search.py runs the cases on the GPU.  Plain numpy and the oracle; nothing here
imports the library under test (c3hlac.synth is numpy only).  The machinery is
generic_search_data.py's, through its case-dict forms.

A search with D <= 160 compresses (compress_kernel over every row of a set_features frame,
compress_rows_body over the listed rows of an extract, compress_f32t_body in the tick; the two
sparse ones up to Dpad = 128), gates every position into a list and projects the listed
positions: score_list_body (VALU, engine 1, r <= 64), score_mfma_kernel<KP> (matrix cores,
engine 2 and every r > 64 single frame), and in the tick score_tick_mfma_body /
score_tick_wide_body.  A D that is no multiple of 4 is padded with zero axes.

Rows follow generic_search_data.rows on the subdivisions (13, 11, 9): small non-negative
integers as float32, about 30 % empty rows, 12 rows with data and exist 0; the exist threshold is
the median box sum of exist.  Cases with r <= 2 add a common component (2 x one random row) to
every row with data, so that no score sits near 0: a single |cos| near 0 carries the absolute
error of any fp32 accumulation at full relative weight.  Bases are synth.random_bases with
synth.whiten; W2 (r > D) takes standard_normal / sqrt(r) model rows, as G8 does.  F8, F18 and W1
(r >= 64) take np_ref.flat_bases with row weights 1, 1/2, 1, 1/2, ...: random_bases' model rows
decay as 0.85^(i/2), and a last row credited to the next model then moves no score by more than
2e-5 to 4e-5 at r = 64 (measured on the float64 scores), so those cases could not see the model
boundaries they are there for.  Seeds moved from the table's 300 + n where a condition of
test_fast_search_data_cpu.py failed: F1, F2 (a smallest score of 0.0004 / 0.0036), F9 (7 passing
boxes over a row with exist 0 and data, 10 wanted), F17 (480 = 15 x 32 listed positions).

case  F    D    M x r    box, rotate    rank  what it reaches
F1    117  4    1 x 1    (2,2,2), off   1     the smallest everything: mfma<16> with 14 zero k-pairs;
                                              the tick's KP = 2 under its 8-pair prefetch; one
                                              16-column window
F2    117  6    3 x 2    (2,2,2), off   1     D padded to 8 by two zero axes, compressed() hands back
                                              6 columns; three models inside one 32-column chunk
F3    117  8    33 x 2   (2,2,2), off   1     VALU mpg = 32: two model groups, the second of one model
F4    300  32   4 x 32   (1,2,3), on    4     top of mfma<16>; last D without the VALU group loop;
                                              mpg 2 with the full 64-column window; models end on
                                              chunk ends; six modes
F5    300  36   7 x 12   (2,2,2), off   1     first D with the group loop; bottom of mfma<24>; groups
                                              of 5 + 2 models straddling 16- and 32-column edges
F6    300  48   2 x 33   (2,2,2), off   1     top of mfma<24>; r = 33: 48-column window, a model
                                              ending one column into the next chunk
F7    300  52   3 x 17   (2,2,2), off   1     bottom of mfma<32>
F8    300  64   2 x 64   (1,2,3), on    2     top of mfma<32>; r = 64 = kOC = D
F9    300  68   5 x 13   (2,2,2), off   1     bottom of mfma<40>; 65 columns: a last chunk of one
                                              column
F10   300  80   1 x 63   (2,2,2), off   1     top of mfma<40>; one model; a window with one padding
                                              column
F11   300  84   9 x 7    (2,2,2), off   1     bottom of mfma<52>; one VALU group of 9 models
F12   981  104  3 x 21   (2,2,2), off   1     top of mfma<52>; feature_max with a zero entry and an
                                              entry equal to a value (G4's construction)
F13   981  108  2 x 40   (2,2,2), off   1     bottom of mfma<64>
F14   981  128  9 x 30   (2,2,2), off   1     top of mfma<64>; last D of the tick and of the sparse
                                              compress, 128 live columns; 270 columns = 9 tiles: two
                                              passes of the tick's MFMA role
F15   981  129  2 x 5    (2,2,2), off   1     padded to 132: first D on the dense compress_kernel's
                                              second column block (4-column tail); bottom of
                                              mfma<72>; a batch of it leaves the tick
F16   981  144  4 x 16   (1,2,3), on    4     top of mfma<72>
F17   981  148  2 x 40   (2,2,2), off   1     bottom of mfma<80>
F18   981  160  9 x 64   (2,2,2), off   1     the largest D of the route on every engine; the window
                                              loop at kQW
W1    981  128  3 x 65   (2,2,2), off   1     the narrowest wide model at the tick's largest D
W2    300  64   2 x 256  (2,2,2), off   1     the widest model score_tick_wide_ok admits (8 tiles)
F19   117  100  6 x 21   (1,2,3), on    1     (18,17,17): 26,014 positions, two model groups of
                                              score_mfma_kernel of 3 models = 63 columns each
W3    981  128  10 x 65  (2,2,2), off   1     four models finish in one pass of the wide role

F19 and W3 are not in the table the route's issue set.  F19: launch_score_mfma_kp splits the models
into the number of groups that its cost model (rounds of resident workgroups x (3 + 32-column
chunks of a group)) finds cheapest.  A list of a few hundred positions is one round whatever the
split, so every case above runs one model per group, or several models inside one chunk (F2, F5,
F9, F11: mfma_groups): the fold never carries ir / m over a chunk edge with a model boundary inside
the chunk, which is what the rows of F5, F6 and F9 name.  With 204 position blocks of 128, six
groups need two rounds on a device of 408 .. 1,223 workgroup slots (MI355X: 256 CUs x 2 .. 4) and
two groups of three models win: model 1 of a group spans columns 21 .. 41 over the chunk edge at 32.
W3: a pass of the wide role is 7 tiles = 224 columns at D = 128, and its third pass (448, 650]
holds the last columns of models 6, 7, 8 and 9 (455, 520, 585, 650): kTickWideFin = 4 finishing
models, the size of the role's score scratch.  W1 finishes three in its one pass, W2 one per three.

References per case: oracle(name), compress64(name), restate32(name) as in
generic_search_data.py; scores64(c, ...) recomputes the float64 scores from compress64, optionally
with one fault (test_fast_search_data_cpu.py: every case sees its own edge).

SPARSE: the inputs of the sparse-compress comparison (compress_rows_body behind an extract
against compress_kernel behind set_features): a 32^3 grid of 5 % occupancy, C3-HLAC-117 on 4^3
subdivisions (512 rows), one projection per D of SPARSE_D.  For D > 117 there is no orthonormal
117 -> D axis; those take standard_normal / sqrt(F) axis rows (any D x F matrix is accepted)."""
import numpy as np

import generic_search_data as gd
import np_ref as npr
import pyoracle as po
from c3hlac import synth
from generic_search_data import SCORE_RTOL_F64, U32  # noqa: F401

SB = (13, 11, 9)
KOC, KFP, KSMC, KSMP, TICK_GX = 64, 32, 32, 128, 16  # search_dev.h / search.hip / pipeline.hip


def _c(F, D, M, r, box, rotate, rank, seed, sb=SB, **kw):
    return dict(F=F, D=D, M=M, r=r, box=box, rotate=rotate, rank=rank, sb=sb, seed=seed, **kw)


CASES = {
    "F1": _c(117, 4, 1, 1, (2, 2, 2), False, 1, 1301, common=2.0),
    "F2": _c(117, 6, 3, 2, (2, 2, 2), False, 1, 1302, common=2.0),
    "F3": _c(117, 8, 33, 2, (2, 2, 2), False, 1, 303, common=2.0),
    "F4": _c(300, 32, 4, 32, (1, 2, 3), True, 4, 304),
    "F5": _c(300, 36, 7, 12, (2, 2, 2), False, 1, 305),
    "F6": _c(300, 48, 2, 33, (2, 2, 2), False, 1, 306),
    "F7": _c(300, 52, 3, 17, (2, 2, 2), False, 1, 307),
    "F8": _c(300, 64, 2, 64, (1, 2, 3), True, 2, 308, flat_q=True),
    "F9": _c(300, 68, 5, 13, (2, 2, 2), False, 1, 1309),
    "F10": _c(300, 80, 1, 63, (2, 2, 2), False, 1, 310),
    "F11": _c(300, 84, 9, 7, (2, 2, 2), False, 1, 311),
    "F12": _c(981, 104, 3, 21, (2, 2, 2), False, 1, 312, with_fmax=True),
    "F13": _c(981, 108, 2, 40, (2, 2, 2), False, 1, 313),
    "F14": _c(981, 128, 9, 30, (2, 2, 2), False, 1, 314),
    "F15": _c(981, 129, 2, 5, (2, 2, 2), False, 1, 315),
    "F16": _c(981, 144, 4, 16, (1, 2, 3), True, 4, 316),
    "F17": _c(981, 148, 2, 40, (2, 2, 2), False, 1, 1317),
    "F18": _c(981, 160, 9, 64, (2, 2, 2), False, 1, 318, flat_q=True),
    "W1": _c(981, 128, 3, 65, (2, 2, 2), False, 1, 319, flat_q=True),
    "W2": _c(300, 64, 2, 256, (2, 2, 2), False, 1, 320, random_q=True),
    "F19": _c(117, 100, 6, 21, (1, 2, 3), True, 1, 321, sb=(18, 17, 17)),
    "W3": _c(981, 128, 10, 65, (2, 2, 2), False, 1, 322, flat_q=True),
}
NAMES = list(CASES)
NARROW = [n for n in NAMES if CASES[n]["r"] <= KOC]  # every engine projects these; bit-identical scores

_CASE, _ORACLE, _C64, _R32 = {}, {}, {}, {}


# ---- the route, restated from the code as plain arithmetic ------------------------------------
def dpad(D):
    """c3h_search_setup: a D <= 160 that is no multiple of 4 gets zero axes up to the next one."""
    return (D + 3) // 4 * 4 if D <= 160 else D


def mfma_kp(D):
    """launch_score_mfma: the instantiation of score_mfma_kernel<KP> for a (padded) D."""
    kp = (dpad(D) + 1) // 2
    return next(k for k in (16, 24, 32, 40, 52, 64, 72, 80) if kp <= k)


def valu_groups(M, r):
    """search_frames: mpg = max(1, 64 / r) models per VALU group -> (mpg, [models per group])."""
    mpg = max(1, KOC // r)
    return mpg, [min(mpg, M - g) for g in range(0, M, mpg)]


def group_loop(D, M, r):
    """launch_tick at engine 1: one workgroup runs every group when the projections fit the window."""
    return len(valu_groups(M, r)[1]) > 1 and dpad(D) * KOC >= KFP * (KOC + 1)


def in_tick(D):
    """search_frames under capture: the tick needs the sparse compress (compress_rows_ok: Dpad <= 128)."""
    return dpad(D) <= 128


def column_blocks(D):
    """compress_kernel: 128-column blocks of the padded D."""
    return -(-dpad(D) // 128)


def tiles_per_model(r):
    """score_tick_tiles(1, r)."""
    return (r + 31) // 32


def _list_lds(D, mpg):
    region = max(D * KFP, KFP * (KOC + 1)) + D * KOC
    return 4 * (region + KFP) + 4 * 4 * KFP + 8 * KFP + 8 * KFP * mpg + 32


def _tick_lds(D, M, r, mpp):
    ft, qv = D * KFP, (KFP + 1) * 32 * ((mpp * r + 31) // 32)
    region = max(ft, qv) if mpp >= M else ft + qv
    return 4 * (region + KFP) + 4 * 4 * KFP + 8 * KFP + 8 * KFP * mpp + 32


def tick_mpp(D, M, r):
    """score_tick_mpp: models per pass of the tick's MFMA role (r <= 64)."""
    D = dpad(D)
    budget = _list_lds(D, valu_groups(M, r)[0])
    mpp = M
    while mpp > 1 and ((mpp * r + 31) // 32 > 8 or _tick_lds(D, M, r, mpp) > budget):
        mpp -= 1
    return mpp


def mfma_groups(ptot, M, r, slots):
    """launch_score_mfma_kp: -> (ngroups, [models per group]) for ptot scheduled positions on a
    device of `slots` resident workgroups."""
    pblocks = -(-ptot // KSMP)
    best, ng = 1e300, 1
    for g in range(1, M + 1):
        rounds = -(-pblocks * g // slots)
        t = rounds * (3.0 + -(-(-(-M // g) * r) // KSMC))
        if t < best:
            best, ng = t, g
    edges = [g * M // ng for g in range(ng + 1)]
    return ng, [b - a for a, b in zip(edges, edges[1:])]


def mfma_straddles(sizes, r):
    """A model boundary strictly inside a 32-column chunk that the group's columns run past:
    the fold then carries ir / m into the next chunk."""
    return any(any((m * r) % KSMC and (m * r) // KSMC < (n * r - 1) // KSMC for m in range(1, n)) for n in sizes)


def _wide_lds(D, tpp):
    return 4 * (D * KFP + (KFP + 1) * 32 * tpp + KFP + 2 * KFP) + 4 * 4 * KFP + 8 * KFP + 8 * KFP * 4 + 32


def wide_tpp(D, M, r):
    """score_tick_wide_tpp: 32-column tiles per pass of the wide role (0: none fits)."""
    D = dpad(D)
    tpp = min((M * r + 31) // 32, 8)
    while tpp > 0 and _wide_lds(D, tpp) > _list_lds(D, 1):
        tpp -= 1
    return tpp


def wide_finishing(D, M, r):
    """[models whose last column a pass holds] per pass of score_tick_wide_body."""
    tpp, C = wide_tpp(D, M, r), M * r
    out = []
    for cA in range(0, C, 32 * tpp):
        cB = min(C, cA + 32 * tpp)
        out.append(sum(1 for m in range(M) if cA < (m + 1) * r <= cB))
    return out


def total_positions(c):
    return sum(e[0] * e[1] * e[2] for _, _, e in gd.modes(c["sb"], c["box"], c["rotate"]))


# ---- cases and references ------------------------------------------------------------------------
def case(name):
    if name not in _CASE:
        _CASE[name] = gd.build_case(CASES[name])
    return _CASE[name]


def oracle(name):
    if name not in _ORACLE:
        c = case(name)
        _ORACLE[name] = gd.oracle_search(c, c["sb"], c["f"], c["ex"], c["rank"])
    return _ORACLE[name]


def compress64(name):
    if name not in _C64:
        _C64[name] = gd.compress64_case(case(name))
    return _C64[name]


def restate32(name):
    if name not in _R32:
        _R32[name] = gd.restate32_case(case(name))
    return _R32[name]


def gates(c):
    """[(P,) bool] per scheduled mode: the positions whose exist box sum passes the threshold."""
    return [b > c["thr"] for b in gd.exist_box_sums(c["sb"], c["ex"], c["box"], c["rotate"])]


def scores64(c, G64, fault=None):
    """Float64 scores from the float64 compress, in the oracle's layout.  fault:
    "last_dim"     the last compressed dimension dropped (a k tail, a padding test off by one)
    "row_to_next"  the last basis row of every model credited to the next model (a model
                   boundary one column late); M > 1
    "last_group"   the last VALU model group's columns zeroed (a window or group not staged)"""
    sb, M, r = c["sb"], c["M"], c["r"]
    G = G64.copy()
    q = c["axis_q"].astype(np.float64)
    if fault == "last_dim":
        G[:, -1] = 0
    if fault == "last_group":
        q = q.copy()
        q[M - valu_groups(M, r)[1][-1]:] = 0
    gv = G.reshape(sb[2], sb[1], sb[0], -1)
    out = []
    for (_, r3, e), gate in zip(gd.modes(sb, c["box"], c["rotate"]), gates(c)):
        fb = gd._box_sum(gv, r3, e)
        p2 = np.einsum("mrd,pd->mrp", q, fb) ** 2
        if fault == "row_to_next":
            assert M > 1
            moved = p2[:, -1].copy()
            p2[:, -1] = 0
            p2[1:, 0] += moved[:-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.sqrt(p2.sum(1)) / np.sqrt((fb * fb).sum(1))[None]
        s[:, ~gate] = -1.0
        out.append(s.reshape(-1))
    return np.concatenate(out)


# ---- the tick's frames ----------------------------------------------------------------------------
TICK_BATCH, TICK_FRAMES = 8, 11  # one full batch and a ragged one
TICK_KINDS = ("rows", "reversed", "empty", "halved")


def tick_kind(i):
    """Frame i of the batch; the cycle starts so that the last frame (10) is the case's own rows,
    whose scores the oracle has."""
    return TICK_KINDS[(i + 2) % 4]


def tick_frame(c, kind):
    """-> (rows, exist) of a frame kind on the case's subdivisions."""
    f, ex = c["f"], c["ex"]
    if kind == "reversed":
        return np.ascontiguousarray(f[::-1]), np.ascontiguousarray(ex[::-1])
    if kind == "empty":
        return np.zeros_like(f), np.zeros_like(ex)
    if kind == "halved":
        f, ex = f.copy(), ex.copy()
        f[::2] = 0
        ex[::2] = 0
    return f, ex


# ---- the sparse compress ----------------------------------------------------------------------------
SPARSE_GRID, SPARSE_S, SPARSE_F, SPARSE_SEED = 32, 4, 117, 41
SPARSE_D = (4, 6, 36, 100, 124, 128)
SPARSE_FMAX_D = 100
SPARSE_BOX = (2, 2, 2)
_SPARSE = {}


def sparse_words():
    if "w" not in _SPARSE:
        _SPARSE["w"] = synth.random_words(SPARSE_GRID, 0.05, seed=SPARSE_SEED)
    return _SPARSE["w"]


def sparse_rows(thr):
    """-> (rows, exist, subdivisions) of the oracle's C3-HLAC-117 on the grid (exact integer mode)."""
    if "rows" not in _SPARSE:
        g, layout, cloud = po.grid_inputs(sparse_words(), (SPARSE_GRID,) * 3, 0.01)
        fe, sb, _ = po.c3hlac(g, layout, cloud, SPARSE_F, thr, 0.01, SPARSE_S, exact=True)
        _SPARSE["rows"] = (fe, po.exist(fe), tuple(int(v) for v in sb))
    return _SPARSE["rows"]


def sparse_setup(D, fe):
    """-> (axis_t, var, axis_q, fmax) of the sparse-compress search at D (2 models of 3 rows)."""
    M, r = 2, min(3, D)
    if D <= SPARSE_F:
        axis_t, var, axis_q = synth.random_bases(SPARSE_F, D, M, r, seed=500 + D)
    else:
        rng = np.random.default_rng(500 + D)
        axis_t = (rng.standard_normal((D, SPARSE_F)) / np.sqrt(SPARSE_F)).astype(np.float32)
        var = (10.0 * 0.93 ** np.arange(D)).astype(np.float32)
        axis_q = npr.flat_bases(D, M, r, 500 + D)
    fmax = (fe.max(0) * np.float32(0.8)).astype(np.float32) if D == SPARSE_FMAX_D else None
    return axis_t, var, axis_q, fmax
