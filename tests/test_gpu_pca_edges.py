"""PCA training (csrc/pca.hip) at its tile and row edges, against sums that leave no tolerance.

The rows of pca_edge_data.py are multiples of 2^-4, so S = sum x x^T over the added vectors
(rotated rows expanded with pca_oracle.rotations24) is the same float64 matrix in whatever order
the MFMA accumulators, the per-split partials, the reduce and the 24-copy gather add it up
(test_pca_edge_data_cpu.py asserts that on the inputs).  Per case, with n the vectors' count:

- mean_flg off: c3h_pca_get_correlation equals S * (1.0 / n) -- P^T S P with a projection of
  entries -1, 0, 1 -- as uint64 views, the one multiply pca_finalize_kernel does;
- mean_flg on: the mean equals float32(sum x * (1.0 / n)) as bytes, and the correlation goes through
  test_gpu_pca.py's _compare (1e-12 of the largest entry: the device may contract the mean
  product into an fma);
- nsample is exact, the variance descending, and eigenvalues and eigenvectors go through _compare
  against numpy's eigh of the same matrix, the project's stated bounds.

Device rows lie in a buffer whose padding columns [F, ld) and whose 32 rows past the last one hold
NaN, host rows with ld > F likewise: a read past a row's F columns or past row n puts a NaN into
the sums.  ld > F goes through c3hlac._capi directly (the binding always passes ld == F).
c3h_rotate_feature90 with ld = dim + 5 writes into a buffer of sentinels and must leave the padding
columns and the rows past n as they were.

_compare cannot take d = 1 (its eigengap looks at a neighbour): _compare_any makes the same
assertions there directly.  The cases and their shapes: pca_edge_data.CASES; the last test counts
the cases that ran against that table."""
import numpy as np
import pytest

import c3hlac
import pca_edge_data as ed
import pca_oracle as pco
from c3hlac._capi import check, ptr
from test_gpu_pca import _compare

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)
GUARD_ROWS = 32
_RAN = {}


@pytest.fixture(scope="module")
def dev(ctx):
    import torch
    return torch.device("cuda", 0)


def _padded(X, ld, guard=GUARD_ROWS):
    """The rows in a NaN buffer of n + guard rows of ld floats."""
    n, F = X.shape
    buf = np.full((n + guard, F if ld is None else ld), np.nan, np.float32)
    buf[:n, :F] = X
    return buf


def _add(pca, a, X, keep, dev):
    import torch
    n, F = X.shape
    if a.where == "dev":
        t = torch.from_numpy(_padded(X, a.ld)).to(dev)
        torch.cuda.synchronize()  # torch's upload before the object's stream reads
        keep.append(t)  # add_data on device rows does not wait for the kernels
        if a.ld is None:
            pca.add_data(t[:n], rotate24=a.rotate)
        else:
            pca._check(pca.lib.c3h_pca_add_data(pca.h, ptr(t), n, a.ld, F, int(a.rotate), 1), "pca_add_data")
    elif a.ld is None:
        pca.add_data(X, rotate24=a.rotate)
    else:
        pca._check(pca.lib.c3h_pca_add_data(pca.h, ptr(_padded(X, a.ld)), n, a.ld, F, int(a.rotate), 0), "pca_add_data")


def _train(case, mean_flg, rows, P, dev, adds=None):
    pca = c3hlac.PCA(mean_flg=mean_flg)
    keep = []
    if P is not None:
        pca.set_compress(P, None, case.D)
    for a, X in zip(case.adds if adds is None else adds, rows):
        _add(pca, a, X, keep, dev)
    pca.solve()  # waits for the stream: the device rows may go
    return pca


def _bits(got, want, tag):
    a, b = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (tag, "entries that differ", len(bad), bad[:6].tolist(),
                           [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]])


def _compare_any(pca, ref, what):
    if len(ref[1]) > 1:
        return _compare(pca, ref, what)
    axis_r, var_r, mean_r, n_r, C_r = ref  # d == 1: _compare's assertions without the eigengap
    assert pca.nsample == n_r, what
    C = pca.correlation()
    assert np.abs(C - C_r).max() <= 1e-12 * np.abs(C_r).max(), what
    np.testing.assert_allclose(pca.variance, var_r.astype(np.float32), rtol=0, atol=1e-9 * var_r[0] + 1e-30)
    assert abs(float(pca.axis[0, 0])) >= 1 - 1e-6 and abs(float(pca.axis[0, 0]) ** 2 - 1) <= 1e-5, what


def _check_exact(pca, want, mean_flg, tag):
    """One solved object against the exact (projected) sums."""
    d = len(want.m)
    assert pca.nsample == want.n, (tag, pca.nsample, want.n)
    assert pca.axis.shape == (d, d) and pca.variance.shape == (d,), tag
    assert (np.diff(pca.variance) <= 0).all(), tag
    inv = 1.0 / want.n
    if mean_flg:
        assert pca.mean.tobytes() == (want.m * inv).astype(np.float32).tobytes(), (tag, "mean")
    else:
        assert pca.mean is None
        _bits(pca.correlation(), want.S * inv, tag)
    _compare_any(pca, ed.reference(want, mean_flg), tag)


def _exact(case, dev):
    rows, P = ed.case_rows(case), ed.case_projection(case)
    want = ed.projected(ed.sums(case, rows), P)
    for mean_flg in case.means:
        tag = (case.name, "mean_flg", mean_flg)
        pca = _train(case, mean_flg, rows, P, dev)
        _check_exact(pca, want, mean_flg, tag)
        if case.kind == "accum":  # one call on the concatenation: the same bytes
            one = _train(case, mean_flg, [np.concatenate(rows)], P, dev, adds=[ed.Add(want.n, False, "host", None)])
            assert one.nsample == pca.nsample and one.correlation().tobytes() == pca.correlation().tobytes(), tag
            assert not mean_flg or one.mean.tobytes() == pca.mean.tobytes(), tag
            one.close()
        if case.kind == "twice":  # a second solve with no new data
            first = (pca.axis.copy(), pca.variance.copy(), pca.mean.copy(), pca.correlation(), pca.nsample)
            pca.solve()
            again = (pca.axis, pca.variance, pca.mean, pca.correlation(), pca.nsample)
            for name, x, y in zip(("axis", "variance", "mean", "correlation"), first, again):
                assert x.tobytes() == y.tobytes(), (tag, "second solve", name)
            assert first[4] == again[4]
            _check_exact(pca, want, mean_flg, tag + ("second solve",))
        pca.close()


def _real(case, dev):
    """_rows-style data against pca_oracle.train: the exact cases do not hang on integer-like rows."""
    (X,), a = ed.case_rows(case), case.adds[0]
    for mean_flg in case.means:
        pca = _train(case, mean_flg, [X], None, dev)
        ref = pco.train(X, rotate=a.rotate, mean_flg=mean_flg)
        _compare(pca, ref, case.name)
        if mean_flg:
            np.testing.assert_allclose(pca.getMean(), ref[2].astype(np.float32), rtol=1e-6)
        pca.close()


def _rot90(case, dev):
    import torch
    a, dim = case.adds[0], case.F
    x = ed.real_rows(a.n, dim, seed=case.seed)
    d_in = torch.from_numpy(_padded(x, a.ld, guard=2)).to(dev)
    for mode in range(4):
        d_out = torch.full((a.n + 2, a.ld), float(SENTINEL), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        check(c3hlac._capi.load().c3h_rotate_feature90(ptr(d_in), ptr(d_out), a.n, a.ld, dim, mode, None), None,
              "rotate_feature90")
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        want = np.ascontiguousarray(pco.rotate_feature90(x, mode), np.float32)
        assert np.ascontiguousarray(out[:a.n, :dim]).tobytes() == want.tobytes(), (case.name, mode)
        assert (out[:a.n, dim:] == SENTINEL).all() and (out[a.n:] == SENTINEL).all(), (case.name, mode, "the sentinel")


@pytest.mark.parametrize("case", ed.CASES, ids=lambda c: c.name)
def test_pca_edge(dev, case):
    {"exact": _exact, "accum": _exact, "twice": _exact, "real": _real, "rot90": _rot90}[case.kind](case, dev)
    _RAN[case.name] = case.group


def test_every_case_ran(dev, request):
    """No case skipped or masked: the cases that ran are the table's, group by group (of a selection
    of this module's tests, every selected case)."""
    picked = {i.callspec.params["case"].name for i in request.session.items
              if i.fspath == request.node.fspath and "case" in getattr(getattr(i, "callspec", None), "params", {})}
    assert picked <= set(_RAN), sorted(picked - set(_RAN))
    if len(picked) == len(ed.CASES):
        groups = {}
        for g in _RAN.values():
            groups[g] = groups.get(g, 0) + 1
        assert groups == ed.GROUP_SIZES and len(_RAN) == len(ed.CASES) == 68
