"""Inputs of test_gpu_pca_edges.py: PCA training rows whose sums are exact, and the table of cases.

No GPU here.  The rows are multiples of 2^-4 in [0, 16) with about 5 % of the columns zero, so every
f32 x f32 product is a multiple of 2^-8 below 2^8 and every sum the device forms -- in the MFMA
accumulators, the per-split partials, the reduce, the 24-copy gather and, with a projection whose
entries are -1, 0 or 1, the two GEMMs -- is an integer multiple of 2^-8 far below 2^53 2^-8: the
float64 result does not depend on the order of the additions.  test_pca_edge_data_cpu.py asserts
that, and every other condition the cases are chosen for, on these inputs with numpy and
oracle/pca_oracle.py alone.

A case is a list of add_data calls on one PCA object (rows, plain or rotate24, host or device rows,
the row stride ld) plus an optional projection.  sums(case) gives S = sum x x^T and m = sum x over
the vectors the reference would add (rotated rows expanded with pca_oracle.rotations24) and their
count n, in float64."""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pca_oracle as pco

TILE = 128  # pca.hip: correlation tile edge over the F + 1 columns (the constant-1 column is index F)

# one add_data call: n rows, rotate24, "dev" or "host" rows, the row stride (None: ld == F)
Add = namedtuple("Add", "n rotate where ld")
# kind: "exact" (integer-like rows, bit patterns), "real" (_rows-style data against pco.train),
# "accum" (exact, and byte-equal to one call on the concatenation), "twice" (exact, solved twice),
# "rot90" (c3h_rotate_feature90 with ld > dim).  means: the mean_flg settings the case runs with.
Case = namedtuple("Case", "name group kind F adds D means seed")


def exact_rows(n, F, seed):
    """n x F float32 rows, multiples of 2^-4 in [0, 16), about 5 % of the columns zero."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, size=(n, F)).astype(np.float32) / np.float32(16)
    X[:, rng.random(F) < 0.05] = 0  # some bins never fire
    return X


def real_rows(n, F, rank=12, seed=0):
    """non-negative feature-like rows with a decaying spectrum (test_gpu_pca.py's _rows)"""
    rng = np.random.default_rng(seed)
    Z = rng.random((n, rank)) * (0.6 ** np.arange(rank))
    B = rng.random((rank, F))
    X = Z @ B + 0.01 * rng.random((n, F))
    X[:, rng.random(F) < 0.05] = 0
    return X.astype(np.float32)


def projection(F, D, seed):
    """F x D float32 with entries in {-1, 0, 1}, no column zero: set_compress(P, None, D)."""
    rng = np.random.default_rng(seed)
    P = rng.integers(-1, 2, size=(F, D)).astype(np.float32)
    P[rng.integers(0, F, size=D), np.arange(D)] = 1
    return P


# ---- the table ------------------------------------------------------------------------------------
SEAM_F = (1, 2, 15, 126, 127, 128, 129, 255, 256, 257, 383, 384, 385)
SEAM_N = 37
ROW_F = 129
ROW_N = (1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 513, 4099)
CAP_F, CAP_N = 2, 1_048_593
LD_N = 300
CHUNK_F, CHUNK_D = 981, 8
CHUNK_N = (17_110, 17_119)
CHUNK_LD = (None, CHUNK_F + 3)  # the second chunk of a strided host buffer starts at rows + r * ld
ACCUM_F = 257
ACCUM_N = (1, 16, 255, 17, 256, 33, 257)
ROT_N, PLAIN_N = 40, 55
COMPRESS_F, COMPRESS_D = 129, (1, 40, 129)
ROT90_DIMS, ROT90_N, ROT90_PAD = (981, 495, 486), (1, 37), 5
GROUP_SIZES = {"tile seams": 26, "row edges": 12, "split cap": 1, "ld device": 4, "ld host": 2, "host chunking": 2,
               "accumulation": 1, "rotate24": 4, "rotate24 + plain": 4, "solve twice": 1, "rotate_feature90": 6,
               "compression": 3, "real-valued": 2}


def _cases():
    out = []

    def add(name, group, kind, F, adds, D=None, means=(False,)):
        out.append(Case(name, group, kind, F, tuple(adds), D, tuple(means), 1000 + len(out)))

    for F in SEAM_F:
        for mean in (False, True):  # device rows without the mean, host rows with it
            add("seam-F%d-%s" % (F, "mean" if mean else "plain"), "tile seams", "exact", F,
                [Add(SEAM_N, False, "host" if mean else "dev", None)], means=(mean,))
    for n in ROW_N:
        add("rows-n%d" % n, "row edges", "exact", ROW_F, [Add(n, False, "dev", None)])
    add("split-cap", "split cap", "exact", CAP_F, [Add(CAP_N, False, "dev", None)])
    for F in (129, 257):
        for ld in (F + 3, 2 * F):
            add("ld-dev-F%d-ld%d" % (F, ld), "ld device", "exact", F, [Add(LD_N, False, "dev", ld)], means=(False, True))
    for ld in (129 + 3, 2 * 129):
        add("ld-host-F129-ld%d" % ld, "ld host", "exact", 129, [Add(LD_N, False, "host", ld)], means=(False, True))
    for n, ld in zip(CHUNK_N, CHUNK_LD):
        add("host-chunk-n%d" % n, "host chunking", "exact", CHUNK_F, [Add(n, False, "host", ld)], D=CHUNK_D)
    add("accumulate", "accumulation", "accum", ACCUM_F,
        [Add(n, False, "host" if k % 2 == 0 else "dev", None) for k, n in enumerate(ACCUM_N)], means=(False, True))
    for F in (495, 486):
        for mean in (False, True):
            add("rot24-F%d-%s" % (F, "mean" if mean else "plain"), "rotate24", "exact", F,
                [Add(ROT_N, True, "dev", None)], means=(mean,))
    for F, D in ((981, 8), (495, None)):
        rot, plain = Add(ROT_N, True, "dev", None), Add(PLAIN_N, False, "host", None)
        add("rot-then-plain-F%d" % F, "rotate24 + plain", "exact", F, [rot, plain], D=D)
        add("plain-then-rot-F%d" % F, "rotate24 + plain", "exact", F, [plain, rot], D=D)
    add("solve-twice", "solve twice", "twice", 129, [Add(LD_N, False, "dev", None)], means=(True,))
    for dim in ROT90_DIMS:
        for n in ROT90_N:
            add("rot90-%d-n%d" % (dim, n), "rotate_feature90", "rot90", dim, [Add(n, False, "dev", dim + ROT90_PAD)])
    for D in COMPRESS_D:
        add("compress-D%d" % D, "compression", "exact", COMPRESS_F, [Add(LD_N, False, "dev", None)], D=D, means=(False, True))
    add("real-F257-mean", "real-valued", "real", 257, [Add(LD_N, False, "dev", None)], means=(True,))
    add("real-F495-rot24", "real-valued", "real", 495, [Add(ROT_N, True, "dev", None)])
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

_CHUNK_ROWS = {}


def case_rows(case):
    """The case's rows, one array per add_data call (views of one draw, in the order of the calls)."""
    total = sum(a.n for a in case.adds)
    if case.kind == "real":
        X = real_rows(total, case.F, seed=case.seed)
    elif case.group == "host chunking":  # the two row counts share one draw: the longer holds the shorter
        if "X" not in _CHUNK_ROWS:
            _CHUNK_ROWS["X"] = exact_rows(max(CHUNK_N), CHUNK_F, 77)
        X = _CHUNK_ROWS["X"][:total]
    elif case.group == "rotate24 + plain":  # either order adds the same rotated and the same plain rows
        Xr, Xp = exact_rows(ROT_N, case.F, 501 + case.F), exact_rows(PLAIN_N, case.F, 502 + case.F)
        return [Xr if a.rotate else Xp for a in case.adds]
    else:
        X = exact_rows(total, case.F, case.seed)
    out, r = [], 0
    for a in case.adds:
        out.append(X[r:r + a.n])
        r += a.n
    return out


def case_projection(case):
    return None if case.D is None else projection(case.F, case.D, 9000 + case.seed)


def expand(rows, rotate):
    """The vectors the reference adds for these rows: the 24 rotations of each, or the rows."""
    return np.concatenate(pco.rotations24(rows), 0) if rotate else rows


Sums = namedtuple("Sums", "S m n")


def sums(case, rows=None):
    """S = sum x x^T, m = sum x, n = the count, over every vector of the case, before any projection."""
    rows = case_rows(case) if rows is None else rows
    F = case.F
    S, m, n = np.zeros((F, F)), np.zeros(F), 0
    for a, X in zip(case.adds, rows):
        V = expand(X, a.rotate).astype(np.float64)
        S += V.T @ V
        m += V.sum(0)
        n += len(V)
    return Sums(S, m, n)


def projected(su, P):
    """G = P^T S P and P^T m: what set_compress(P, None, D) makes the solve decompose."""
    if P is None:
        return su
    P = P.astype(np.float64)
    return Sums(P.T @ su.S @ P, P.T @ su.m, su.n)


def reference(su, mean_flg):
    """pca.cpp:80-105 on exact sums, as pca_oracle.train returns it:
    (axis, variance, mean or None, nsample, the correlation the solve decomposes)."""
    inv = 1.0 / su.n
    C = su.S * inv
    mean = None
    if mean_flg:
        mean = su.m * inv
        C = C - np.outer(mean, mean)
    w, V = np.linalg.eigh(C)
    order = pco.sort_desc(w)
    return V[:, order], w[order], mean, su.n, C


# ---- integer arithmetic for the CPU conditions ------------------------------------------------------
def scaled(X):
    """The rows times 16 as int64; they are integers in [0, 256)."""
    Xi = np.rint(X.astype(np.float64) * 16).astype(np.int64)
    assert np.array_equal(Xi.astype(np.float64) / 16, X.astype(np.float64)) and ((Xi >= 0) & (Xi < 256)).all()
    return Xi


def int_gram(Xi):
    """Xi^T Xi in int64 (numpy has no BLAS for integers: by column blocks, upper triangle, in threads)."""
    A = np.ascontiguousarray(Xi.T)
    F = A.shape[0]
    edges = list(range(0, F, TILE)) + [F]
    G = np.zeros((F, F), np.int64)

    def block(ij):
        i, j = ij
        a, b = A[edges[i]:edges[i + 1]], A[edges[j]:edges[j + 1]]
        return i, j, np.einsum("ik,jk->ij", a, b)

    pairs = [(i, j) for i in range(len(edges) - 1) for j in range(i, len(edges) - 1)]
    with ThreadPoolExecutor(8) as ex:
        for i, j, g in ex.map(block, pairs):
            G[edges[i]:edges[i + 1], edges[j]:edges[j + 1]] = g
            G[edges[j]:edges[j + 1], edges[i]:edges[i + 1]] = g.T
    return G


def augmented_tiles(S, m, n):
    """The 128 x 128 tiles (bi <= bj) of one accumulator: sum x x^T over the F + 1 columns."""
    F = len(m)
    nb = (F + 1 + TILE - 1) // TILE
    A = np.zeros((nb * TILE, nb * TILE))
    A[:F, :F] = S
    A[:F, F] = A[F, :F] = m
    A[F, F] = n
    return {(i, j): A[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE] for i in range(nb) for j in range(i, nb)}


def rotation_maps(dim):
    """The 24 gather maps of pca_oracle.rotations24 on this dimension, 24 x dim."""
    return np.stack(pco.rotations24(np.arange(dim)))
