"""Cases and references for the generic search route (D > 160): test_generic_search_data_cpu.py
checks the inputs and the references against each other, test_gpu_generic_search.py runs the
cases on the GPU.  Plain numpy and the oracle; nothing here imports the library under test
(c3hlac.synth is numpy only).

A search whose compressed dimension is above 160 takes none of the gate-list routes: it runs
compress_kernel over every row, score_kernel<64> (D <= 256) or score_kernel<16> (D > 256) over
every position, and replay_kernel.

Frames are feature rows for Context.set_features: small non-negative integers as float32, about
30 % of the rows all zero.  exist is passed explicitly: positive on the rows with data except a
few (EXIST0_ROWS), whose 0 must not keep their data out of the box sums.  Compressed cases take
synth.random_bases with synth.whiten; the uncompressed case (identity projection) draws its
model rows from standard_normal.  The exist threshold is the median of the box sums of exist over
the scheduled modes.

case   F    D     M x r   box, rotate      rank  subdivisions  what it reaches
G1     300  164   3 x 5   (2,2,2), off     1     (9,7,6)       first D past the fast route; second
                                                               column block with a 4-column tail
G2     300  236   3 x 70  (1,2,3), on      4     (9,7,6)       r > 64 with r % 4 != 0; six modes
G3     300  256   2 x 20  (1,2,3), off     1     (9,7,6)       last D of score_kernel<64>; 71,424 B LDS
G4     300  260   2 x 20  (1,2,3), on      2     (9,7,6)       first D of score_kernel<16>; feature_max
                                                               with a zero and an entry equal to a value
G5     981  981   2 x 70  (1,2,3), off     1     (9,7,6)       uncompressed: identity PT, 8 column
                                                               blocks, 67,456 B LDS; feature_max
G6     200  165   1 x 3   (2,1,1), on      1     (7,5,4)       D no multiple of 4 and not padded
                                                               (Dpad 168); F % 128 = 72; r below both
                                                               kernels' rows per pass
G7     300  300   1 x 3   (2,2,2), off     1     (7,5,4)       score_kernel<16> with r < 16

G8     300  164   1 x 480 (1,2,3), off     1     (9,7,6)       D <= 256 on score_kernel<16>: 64
                                                               positions do not fit the LDS

G8: score_kernel<64> asks for 256 * (D + r + 3) B of LDS, 165,632 B here, more than the 163,840 B a
workgroup gets on gfx950, so the launch takes score_kernel<16> (41,408 B) although D <= 256
(score_generic_sp).  Its 480 model rows of 164 floats are standard_normal / sqrt(r): more rows than
dimensions, no orthonormal set.  Not in the table the route's issue set; it covers the one path
the LDS check added.

G7 runs on G6's subdivisions: on (9,7,6) its one mode has 8 * 6 * 5 = 240 = 15 * 16 positions, a
whole number of score_kernel<16> workgroups, and every case must leave a partial last workgroup
in some mode (here 6 * 4 * 3 = 72 = 4 * 16 + 8).

References per case (by name, cached; build_case, compress64_case, restate32_case and
box_norms64_case take a case dict: fast_search_data.py shares them):
  oracle(name)      the float64 oracle (pyoracle.search, dbl=True): lists and scores
  compress64(name)  float64 compress of the rows as setData normalises them (float32 division,
                    search.cpp:563-570), and the forward bound of a length-F fp32 chain
  restate32(name)   the route restated in fp32: compress chain in ascending j, box sums in
                    (dz, dy, dx) order, the norm and each projection as chains in ascending d,
                    sqrt and divide in double.  It exists to show that SCORE_RTOL_F64 is within
                    reach of a faithful fp32 kernel; the GPU is never compared with it.
"""
import numpy as np

import np_ref as npr
import pyoracle as po
from c3hlac import synth

SCORE_RTOL_F64 = 1e-5  # tests/test_gpu_parity.py: GPU (fp32, direct box sums) vs the float64 oracle
U32 = 2.0 ** -24       # unit roundoff of float32
EXIST0_ROWS = 12       # rows with data whose exist is 0

CASES = {
    "G1": dict(F=300, D=164, M=3, r=5, box=(2, 2, 2), rotate=False, rank=1, sb=(9, 7, 6), seed=101),
    "G2": dict(F=300, D=236, M=3, r=70, box=(1, 2, 3), rotate=True, rank=4, sb=(9, 7, 6), seed=102),
    "G3": dict(F=300, D=256, M=2, r=20, box=(1, 2, 3), rotate=False, rank=1, sb=(9, 7, 6), seed=103),
    "G4": dict(F=300, D=260, M=2, r=20, box=(1, 2, 3), rotate=True, rank=2, sb=(9, 7, 6), seed=104, with_fmax=True),
    "G5": dict(F=981, D=981, M=2, r=70, box=(1, 2, 3), rotate=False, rank=1, sb=(9, 7, 6), seed=105, with_fmax=True,
               uncompressed=True),
    "G6": dict(F=200, D=165, M=1, r=3, box=(2, 1, 1), rotate=True, rank=1, sb=(7, 5, 4), seed=106),
    "G7": dict(F=300, D=300, M=1, r=3, box=(2, 2, 2), rotate=False, rank=1, sb=(7, 5, 4), seed=107),
    "G8": dict(F=300, D=164, M=1, r=480, box=(1, 2, 3), rotate=False, rank=1, sb=(9, 7, 6), seed=108, random_q=True),
}
LDS_PER_WORKGROUP = 163840  # gfx950 (hipDeviceAttributeMaxSharedMemoryPerBlock)
NAMES = sorted(CASES)

_CASE, _ORACLE, _C64, _R32 = {}, {}, {}, {}


def positions_per_workgroup(D, r):
    """score_kernel<64> up to D = 256 where its 256 * (D + r + 3) B of LDS fit, score_kernel<16> else."""
    return 64 if D <= 256 and 256 * (D + r + 3) <= LDS_PER_WORKGROUP else 16


def rows(sb, F, rng, common=0.0):
    """-> (rows, exist): small integers, ~30 % empty rows, EXIST0_ROWS rows with data and exist 0.
    common: every row with data also gets common x one random row (search_fp16_cases.COMMON's
    device: it keeps the scores of r <= 2 models away from 0)."""
    H = int(np.prod(sb))
    f = np.floor(rng.random((H, F)) * 4).astype(np.float32)
    if common:
        f = f + np.float32(common) * rng.random(F, dtype=np.float32)[None, :]
    f[rng.random(H) < 0.3] = 0
    live = np.flatnonzero(f.any(1))
    ex = np.zeros(H, np.int32)
    ex[live] = rng.integers(1, 10, live.size)
    ex[rng.choice(live, EXIST0_ROWS, replace=False)] = 0
    return f, ex


def bases(c):
    """-> (axis_t, var, axis_q) of a case (axis_t, var None: no compression)."""
    if c.get("uncompressed"):
        rng = np.random.default_rng(c["seed"] + 1000)
        return None, None, rng.standard_normal((c["M"], c["r"], c["D"])).astype(np.float32)
    if c.get("random_q"):  # more model rows than dimensions: any M x r x D is accepted
        axis_t, var, _ = synth.random_bases(c["F"], c["D"], 1, 1, seed=c["seed"])
        rng = np.random.default_rng(c["seed"] + 1000)
        return axis_t, var, (rng.standard_normal((c["M"], c["r"], c["D"])) / np.sqrt(c["r"])).astype(np.float32)
    if c.get("flat_q"):
        # model rows of weight 1, 1/2, 1, 1/2, ... on np_ref.flat_bases: random_bases' rows decay as
        # 0.85^(i/2), which hides a model's last rows below 1e-4 of the score from r of about 40;
        # unweighted, r = D would score 1 everywhere
        axis_t, var, _ = synth.random_bases(c["F"], c["D"], 1, 1, seed=c["seed"])
        w = np.where(np.arange(c["r"]) % 2, np.float32(0.5), np.float32(1))
        return axis_t, var, (npr.flat_bases(c["D"], c["M"], c["r"], c["seed"] + 1) * w[None, :, None]).astype(np.float32)
    return synth.random_bases(c["F"], c["D"], c["M"], c["r"], seed=c["seed"])


def modes(sb, box, rotate):
    """[(mode, (xr, yr, zr), (xe, ye, ze))] of the scheduled modes whose box fits."""
    out = []
    for mode in npr.mode_schedule(box, rotate):
        xr, yr, zr = npr._ranges(mode, box)
        e = (sb[0] - xr + 1, sb[1] - yr + 1, sb[2] - zr + 1)
        if min(e) > 0:
            out.append((mode, (xr, yr, zr), e))
    return out


def _box_sum(vol, rng3, ext):
    """Direct box sums in (dz, dy, dx) order, in vol's dtype; vol[z, y, x, ...]."""
    (xr, yr, zr), (xe, ye, ze) = rng3, ext
    s = np.zeros((ze, ye, xe) + vol.shape[3:], vol.dtype)
    for dz in range(zr):
        for dy in range(yr):
            for dx in range(xr):
                s = s + vol[dz:dz + ze, dy:dy + ye, dx:dx + xe]
    return s.reshape((ze * ye * xe,) + vol.shape[3:])


def exist_box_sums(sb, ex, box, rotate):
    """The integer box sums of exist, every scheduled mode, scan order."""
    ev = ex.astype(np.int64).reshape(sb[2], sb[1], sb[0])
    return [_box_sum(ev, r3, e) for _, r3, e in modes(sb, box, rotate)]


def threshold(sb, ex, box, rotate):
    return int(np.median(np.concatenate(exist_box_sums(sb, ex, box, rotate))))


def normalise(f, fmax):
    """setData's histogram normalisation in float32 (search.cpp:563-570)."""
    if fmax is None:
        return f
    fm = np.asarray(fmax, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (f / fm[None, :]).astype(np.float32)
    return np.where(fm[None, :] == 0, np.float32(0), np.where(f == fm[None, :], np.float32(1), q)).astype(np.float32)


def build_case(row):
    """The inputs of a table row: the row plus f, ex, axis_t, var, ap (whitened, None when
    uncompressed), axis_q, fmax (None without) and thr."""
    c = dict(row)
    rng = np.random.default_rng(c["seed"])
    c["f"], c["ex"] = rows(c["sb"], c["F"], rng, c.get("common", 0.0))
    c["axis_t"], c["var"], c["axis_q"] = bases(c)
    c["ap"] = None if c["axis_t"] is None else synth.whiten(c["axis_t"], c["var"])
    c["fmax"] = None
    if c.get("with_fmax"):
        fm = rng.integers(2, 6, c["F"]).astype(np.float32)  # 3: equal to values of that column
        fm[7] = 0
        c["fmax"] = fm
    c["thr"] = threshold(c["sb"], c["ex"], c["box"], c["rotate"])
    return c


def case(name):
    if name not in _CASE:
        _CASE[name] = build_case(CASES[name])
    return _CASE[name]


def oracle_search(c, sb, f, ex, rank):
    """-> (Lists, scores) of the float64 oracle for rows f / exist ex on subdivisions sb."""
    L, _, sc = po.search(sb, f, ex, c["ap"], c["axis_q"], c["box"], rank, c["thr"], rotate=c["rotate"], dbl=True,
                         fmax=c["fmax"], want_scores=True)
    return L, sc


def oracle(name):
    if name not in _ORACLE:
        c = case(name)
        _ORACLE[name] = oracle_search(c, c["sb"], c["f"], c["ex"], c["rank"])
    return _ORACLE[name]


def compress64_rows(f, ap, fmax):
    """-> (G64, bound): G64 = fn @ ap^T in float64 (fn: the float32-normalised rows), and the
    elementwise bound on a float32 fma chain of length F against it, gamma_F * (|fn| @ |ap|^T) with
    gamma_F = F u / (1 - F u), plus u * |G64| for the rounding of G64 itself to float32."""
    fn = normalise(f, fmax).astype(np.float64)
    F = f.shape[1]
    if ap is None:
        G, mag = fn, np.abs(fn)
    else:
        ap = ap.astype(np.float64)
        G, mag = fn @ ap.T, np.abs(fn) @ np.abs(ap).T
    g = F * U32 / (1 - F * U32)
    return G, g * mag + U32 * np.abs(G)


def compress64_case(c):
    return compress64_rows(c["f"], c["ap"], c["fmax"])


def compress64(name):
    if name not in _C64:
        _C64[name] = compress64_case(case(name))
    return _C64[name]


def _fma32(a, b, acc):
    """float32 fma(a, b, acc): the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def restate32(name):
    if name not in _R32:
        _R32[name] = restate32_case(case(name))
    return _R32[name]


def restate32_case(c):
    """The route in fp32 -> scores in the oracle's layout (mode, model, position)."""
    sb, M, r, D = c["sb"], c["M"], c["r"], c["D"]
    fn = normalise(c["f"], c["fmax"])
    if c["ap"] is None:
        G = fn
    else:
        G = np.zeros((fn.shape[0], D), np.float32)
        for j in range(c["F"]):  # ascending j
            G = _fma32(fn[:, j:j + 1], c["ap"][None, :, j], G)
    gv = G.reshape(sb[2], sb[1], sb[0], D)
    ev = c["ex"].astype(np.int64).reshape(sb[2], sb[1], sb[0])
    q = c["axis_q"].reshape(M * r, D)
    out = []
    for _, r3, e in modes(sb, c["box"], c["rotate"]):
        gate = _box_sum(ev, r3, e) > c["thr"]
        fb = _box_sum(gv, r3, e)  # float32 adds from 0 in (dz, dy, dx) order
        P = fb.shape[0]
        ff = np.zeros(P, np.float32)
        t = np.zeros((M * r, P), np.float32)
        for d in range(D):  # ascending d
            ff = _fma32(fb[:, d], fb[:, d], ff)
            t = _fma32(q[:, d:d + 1], fb[None, :, d], t)
        t = t.reshape(M, r, P)
        q2 = np.zeros((M, P), np.float32)
        for i in range(r):
            q2 = _fma32(t[:, i], t[:, i], q2)
        with np.errstate(divide="ignore", invalid="ignore"):
            sc = np.sqrt(q2.astype(np.float64)) / np.sqrt(ff.astype(np.float64))[None, :]
        sc[:, ~gate] = -1.0
        out.append(sc.reshape(-1))
    return np.concatenate(out)


def box_norms64(name):
    return box_norms64_case(case(name), compress64(name)[0])


def box_norms64_case(c, G64):
    """Float64 norms of the compressed box rows, every scheduled mode (scan order)."""
    sb = c["sb"]
    gv = G64.reshape(sb[2], sb[1], sb[0], -1)
    return [np.sqrt((_box_sum(gv, r3, e) ** 2).sum(1)) for _, r3, e in modes(sb, c["box"], c["rotate"])]


def mode_blocks(sc, M, sb, box, rotate):
    """Scores in the c3h_get_scores layout -> [(mode, (M, P) view)] per scheduled mode."""
    out, off = [], 0
    for mode, _, e in modes(sb, box, rotate):
        P = e[0] * e[1] * e[2]
        out.append((mode, sc[off:off + M * P].reshape(M, P)))
        off += M * P
    assert off == sc.size
    return out


# ---- batch entry points: three feature frames on G1's and on G4's bases ------------------
# (9,7,1) holds a (1,2,3) box in two of the six modes only (those with zr = 1)
BATCH_SUBDIVS = [(9, 7, 6), (7, 5, 4), (9, 7, 1)]
BATCH_BOX, BATCH_ROTATE, BATCH_RANK = (1, 2, 3), True, 2
_BATCH = {}


def batch_frames():
    """[(subdivisions, rows, exist)] of the three frames (F = 300, shared by both bases)."""
    if "frames" not in _BATCH:
        _BATCH["frames"] = [(sb,) + rows(sb, 300, np.random.default_rng(210 + i)) for i, sb in enumerate(BATCH_SUBDIVS)]
    return _BATCH["frames"]


def batch_case(name):
    """The bases of case `name` with the batch's box, rotation and rank; one threshold for the
    three frames (the median over all of their exist box sums)."""
    if name not in _BATCH:
        c = dict(case(name))
        c["box"], c["rotate"], c["rank"] = BATCH_BOX, BATCH_ROTATE, BATCH_RANK
        c["thr"] = int(np.median(np.concatenate([b for sb, _, ex in batch_frames()
                                                 for b in exist_box_sums(sb, ex, BATCH_BOX, BATCH_ROTATE)])))
        _BATCH[name] = c
    return _BATCH[name]


def batch_oracle(name, i):
    if (name, i) not in _BATCH:
        sb, f, ex = batch_frames()[i]
        _BATCH[name, i] = oracle_search(batch_case(name), sb, f, ex, BATCH_RANK)
    return _BATCH[name, i]


# ---- list state on both routes: G2 (generic) and G1's rows at D = 40 (fast), rank 4 ----------
def list_state_case(route):
    if ("ls", route) not in _BATCH:
        if route == "generic":
            c = dict(case("G2"))
        else:
            c = dict(case("G1"))
            c["D"], c["box"], c["rotate"], c["rank"] = 40, (1, 2, 3), True, 4
            c["axis_t"], c["var"], c["axis_q"] = synth.random_bases(c["F"], 40, c["M"], c["r"], seed=c["seed"] + 1)
            c["ap"] = synth.whiten(c["axis_t"], c["var"])
            c["thr"] = threshold(c["sb"], c["ex"], c["box"], c["rotate"])
        _BATCH["ls", route] = c
    return _BATCH["ls", route]
