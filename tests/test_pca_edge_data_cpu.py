"""The inputs of test_gpu_pca_edges.py without a GPU: numpy and oracle/pca_oracle.py alone show that
every case's sums are exact in float64 whatever the order of the additions, that a swapped or
transposed tile and an idle rotation fold would change them, and that the row counts sit where the
cases are meant to sit relative to the 16-row stage, the 256-row split, the 4,096-block cap and the
64 MB host chunk.  These are conditions on the inputs, not tolerances."""
import numpy as np
import pytest

import pca_edge_data as ed
import pca_oracle as pco

TRAINED = [c for c in ed.CASES if c.kind != "rot90"]
EXACT = [c for c in TRAINED if c.kind != "real"]
_INT = {}


def _int_sums(case):
    """sum x x^T and sum x over the case's vectors in int64, on the rows times 16."""
    key = (case.group, case.F) if case.group in ("host chunking", "rotate24 + plain") else case.name
    if case.group == "host chunking":  # the longer row count holds the shorter: add the last rows to its sums
        X = ed.case_rows(case)[0]
        short = min(ed.CHUNK_N)
        if key not in _INT:
            _INT[key] = ed.int_gram(ed.scaled(X[:short]))
        tail = ed.scaled(X[short:])
        return _INT[key] + tail.T @ tail, ed.scaled(X).sum(0)
    if key not in _INT:
        V = np.concatenate([ed.scaled(ed.expand(X, a.rotate)) for a, X in zip(case.adds, ed.case_rows(case))])
        _INT[key] = (ed.int_gram(V), V.sum(0))
    return _INT[key]


def test_the_table_has_every_group():
    got = {}
    for c in ed.CASES:
        got[c.group] = got.get(c.group, 0) + 1
    assert got == ed.GROUP_SIZES and len(ed.CASES) == 68 and len(ed.BY_NAME) == 68
    assert sorted({c.F for c in ed.CASES if c.group == "tile seams"}) == [1, 2, 15, 126, 127, 128, 129, 255, 256, 257, 383, 384, 385]
    assert all(c.adds[0].n == 37 for c in ed.CASES if c.group == "tile seams")
    assert sum(c.means == (True,) for c in ed.CASES if c.group == "tile seams") == 13
    assert [c.adds[0].n for c in ed.CASES if c.group == "row edges"] == [1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 513, 4099]
    assert all((c.F if c.D is None else c.D) <= 495 for c in TRAINED)  # the eigensolve's width


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_sums_are_exact(case):
    """X^T X in float64 equals the int64 product of the rows times 16, divided by 256, below 2^53;
    with a projection of entries -1, 0, 1 so does P^T S P, whose every partial sum is bounded by
    |P|^T S |P|."""
    rows = ed.case_rows(case)
    for X in rows:
        assert X.dtype == np.float32 and X.min() >= 0 and X.max() < 16
        zero = (X == 0).all(0).mean()
        assert zero <= 0.12, zero  # about 5 % of the columns
    su = ed.sums(case, rows)
    Si, mi = _int_sums(case)
    assert 0 < Si.max() < 2 ** 53 and su.n == sum(a.n * (24 if a.rotate else 1) for a in case.adds)
    assert np.array_equal(su.S, Si.astype(np.float64) / 256)
    assert np.array_equal(su.m, mi.astype(np.float64) / 16)
    P = ed.case_projection(case)
    if P is None:
        return
    assert P.shape == (case.F, case.D) and set(np.unique(P).tolist()) <= {-1.0, 0.0, 1.0} and np.abs(P).sum(0).min() >= 1
    Pi = P.astype(np.int64)
    assert (np.abs(Pi).T @ Si @ np.abs(Pi)).max() < 2 ** 53
    pr = ed.projected(su, P)
    assert np.array_equal(pr.S, (Pi.T @ Si @ Pi).astype(np.float64) / 256)
    assert np.array_equal(pr.m, (Pi.T @ mi).astype(np.float64) / 16)
    assert np.abs(pr.S).max() > 0 and len(np.unique(pr.S)) > case.D * (case.D + 1) // 4


@pytest.mark.parametrize("case", TRAINED, ids=lambda c: c.name)
def test_a_swapped_or_transposed_tile_changes_the_sums(case):
    """Per accumulator (the plain rows', the rotated rows' raw rows) of more than one tile block: no
    two of its 128 x 128 tiles are equal and no off-diagonal tile equals its own transpose."""
    nb = (case.F + 1 + ed.TILE - 1) // ed.TILE
    if nb == 1:
        assert case.F <= 127
        return
    rows = ed.case_rows(case)
    for rotate in (False, True):
        X = [x for a, x in zip(case.adds, rows) if a.rotate == rotate]
        if not X:
            continue
        X = np.concatenate(X).astype(np.float64)
        tiles = ed.augmented_tiles(X.T @ X, X.sum(0), len(X))
        assert len(tiles) == nb * (nb + 1) // 2
        keys = sorted(tiles)
        for a, ka in enumerate(keys):
            assert np.abs(tiles[ka]).max() > 0, ka
            if ka[0] != ka[1]:
                assert not np.array_equal(tiles[ka], tiles[ka].T), ka
            for kb in keys[a + 1:]:
                assert not np.array_equal(tiles[ka], tiles[kb]), (ka, kb)
                assert not np.array_equal(tiles[ka], tiles[kb].T), (ka, kb)


def test_tile_block_counts():
    """F + 1 columns in 128-column blocks: 127 ends on a tile, 128 / 256 / 384 leave the ones column
    alone in the last one; nb = 1 .. 4 among the seams, 8 at 981."""
    nb = {F: -(-(F + 1) // 128) for F in ed.SEAM_F + (981, 495, 486)}
    assert (127 + 1) % 128 == 0 and all((F + 1) % 128 == 1 for F in (128, 256, 384))
    assert [nb[F] for F in ed.SEAM_F] == [1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
    assert nb[981] == 8 and nb[495] == 4 and nb[486] == 4 and -(-(ed.ROW_F + 1) // 128) == 2


def test_row_counts_sit_on_the_stage_split_and_cap_edges():
    assert ed.SEAM_N == 2 * 16 + 5
    n = ed.ROW_N
    assert n[:2] == (1, 2) and n[1] < 16  # less than one stage
    assert n[2:7] == (16 - 1, 16, 16 + 1, 2 * 16 - 1, 2 * 16 + 1)  # either side of one and of two stages
    assert n[7:11] == (256 - 1, 256, 256 + 1, 2 * 256 + 1)  # either side of a split; a second and a third split of one row
    assert n[11] == 16 * 256 + 3 and 3 % 16 != 0  # seventeen splits, the last one's tail no whole stage
    # the cap: one tile pair (F + 1 = 3 columns), 4,096 blocks at the most; 256-row splits would need 4,097
    assert ed.CAP_F + 1 <= 128 and ed.CAP_N == 4096 * 256 + 17 and -(-ed.CAP_N // 256) == 4097 > 4096
    assert -(-ed.CAP_N // 4096) == 257 > 256  # so a block takes more than 256 rows: several stages of its own tail
    assert ed.CAP_N * 24 * 2 ** 16 < 2 ** 53
    assert ed.ACCUM_N == (1, 16, 255, 17, 256, 33, 257) and sum(ed.ACCUM_N) == 835
    assert ed.LD_N == 256 + 2 * 16 + 12


def test_host_chunk_is_exceeded():
    chunk = (64 << 20) // (4 * ed.CHUNK_F)
    assert chunk == 17_102
    assert ed.CHUNK_N[0] == 17_110 > chunk and ed.CHUNK_N[0] - chunk == 8 < 16  # a second chunk of half a stage
    assert ed.CHUNK_N[1] == chunk + 16 + 1  # a second chunk of one stage and one row
    assert all(c.D == 8 and c.adds[0].where == "host" for c in ed.CASES if c.group == "host chunking")
    # the stated case through the binding (ld == F); the longer one strided, so that the second
    # chunk's start depends on ld
    assert [c.adds[0].ld for c in ed.CASES if c.group == "host chunking"] == [None, ed.CHUNK_F + 3]


def test_strides_and_places():
    """ld > F on device and on host rows at both stated strides; host and device rows alternate in
    the accumulation; rotate_feature90 runs with ld = dim + 5."""
    ld = {(c.F, c.adds[0].where, c.adds[0].ld) for c in ed.CASES if c.group in ("ld device", "ld host")}
    assert ld == {(129, "dev", 132), (129, "dev", 258), (257, "dev", 260), (257, "dev", 514), (129, "host", 132), (129, "host", 258)}
    acc = ed.BY_NAME["accumulate"]
    assert [a.where for a in acc.adds] == ["host", "dev"] * 3 + ["host"]
    assert {(c.F, c.adds[0].n, c.adds[0].ld - c.F) for c in ed.CASES if c.kind == "rot90"} == {
        (d, n, 5) for d in (981, 495, 486) for n in (1, 37)}
    orders = [[a.rotate for a in c.adds] for c in ed.CASES if c.group == "rotate24 + plain"]
    assert orders == [[True, False], [False, True]] * 2
    assert [(c.F, c.D) for c in ed.CASES if c.group == "rotate24 + plain"] == [(981, 8), (981, 8), (495, None), (495, None)]
    assert [(c.F, c.D) for c in ed.CASES if c.group == "compression"] == [(129, 1), (129, 40), (129, 129)]


@pytest.mark.parametrize("dim", [981, 495, 486])
def test_the_rotation_fold_has_work_to_do(dim):
    maps = ed.rotation_maps(dim)
    assert maps.shape == (24, dim) and all(sorted(m.tolist()) == list(range(dim)) for m in maps)
    assert len({m.tobytes() for m in maps}) == 24  # pairwise different
    if dim == 981:  # both halves move
        assert all((m[:495] != np.arange(495)).any() and (m[495:] != np.arange(495, 981)).any() for m in maps[1:])
    for case in ed.CASES:
        if case.F != dim or case.kind == "rot90" or not any(a.rotate for a in case.adds):
            continue
        X = np.concatenate([x for a, x in zip(case.adds, ed.case_rows(case)) if a.rotate]).astype(np.float64)
        S = X.T @ X
        fold = sum(S[np.ix_(m, m)] for m in maps)
        assert not np.array_equal(fold, 24 * S), case.name
        if case.kind != "real":  # exact rows: the fold of the raw sums is the sum over the expanded rows, bit for bit
            only = case._replace(adds=tuple(a for a in case.adds if a.rotate))
            assert np.array_equal(fold, ed.sums(only, [x for a, x in zip(case.adds, ed.case_rows(case)) if a.rotate]).S), case.name
        # the mean column folds too: sum_k P_k m differs from 24 m
        assert not np.array_equal(sum(X.sum(0)[m] for m in maps), 24 * X.sum(0)), case.name


def test_real_rows_are_not_integer_like():
    for case in ed.CASES:
        if case.kind == "real":
            X = ed.case_rows(case)[0]
            assert X.dtype == np.float32 and (X * 16 != np.rint(X * 16)).mean() > 0.8
    assert [(c.F, c.means, c.adds[0].rotate) for c in ed.CASES if c.kind == "real"] == [(257, (True,), False), (495, (False,), True)]


def test_reference_matches_the_oracle():
    """ed.reference on the exact sums is pca_oracle.train on the same rows, up to float64 rounding."""
    case = ed.BY_NAME["rot24-F486-mean"]
    X = ed.case_rows(case)[0][:6]
    small = case._replace(adds=(ed.Add(6, True, "dev", None),))
    a, w, mean, n, C = ed.reference(ed.sums(small, [X]), True)
    a2, w2, mean2, n2, C2 = pco.train(X, rotate=True, mean_flg=True)
    assert n == n2 == 144 and np.allclose(C, C2, rtol=0, atol=1e-12 * np.abs(C2).max())
    assert np.allclose(mean, mean2, rtol=1e-14) and np.allclose(w, w2, rtol=0, atol=1e-10 * w2[0])
