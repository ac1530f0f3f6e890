"""c3h_pca_add_c3_frames (point clouds in, PCA::addData of every C3-HLAC row with exist > 0 out: the
packed pass of csrc/c3_sparse.hip per batch into a buffer of the context, then the device path of
c3h_pca_add_data) against oracle/pca_oracle.py on the oracle's packed rows.

The bound is test_gpu_pca.py's own: the correlation the solve decomposes within 1e-12 x max|C| of
pca_oracle.train, which holds because the device sums are f64 of exact f32 x f32 products and the
rows are, bit for bit, the oracle's (test_gpu_packed_rows.py).  The clouds are mixed_boxes (64
frames, 1,067 rows, 12 frames without a row: packed_rows_data.py).  Variant 117 plain; variant 981
with set_compress (a seeded orthonormal axis, D = 20, seeded variances) and rotate24 against
train(..., rotate=True, exact=True).  The result equals add_data on the packed tensor, set_batch(5)
equals set_batch(64), a context and a PCA object on streams of their own give the same, all within
that bound.  Errors: rotate24 at 117 and a differing F fail as c3h_pca_add_data does and enqueue
nothing; a bad variant is C3H_ERR_ARG."""
import numpy as np
import pytest

import c3_rows_data as rd
import c3_sparse_data as sd
import c3hlac
import packed_rows_data as pd_
import pca_oracle as pco
from c3hlac import _capi
from conftest import THR

pytestmark = pytest.mark.gpu
BOUND = 1e-12
N = 1067
D = 20
ARGS = dict(subdiv=sd.MIXED_SUBDIV, offset=sd.MIXED_OFFSET, color_mode=sd.CM)


@pytest.fixture(scope="module")
def hctx():
    c = c3hlac.Context(0)
    c.set_batch(64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def clouds():
    return list(sd.mixed_boxes())


@pytest.fixture(scope="module")
def packed117(clouds):
    return pd_.packed(clouds, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, 117)


@pytest.fixture(scope="module")
def ref117(packed117):
    return pco.train(packed117.rows)


@pytest.fixture(scope="module")
def compress():
    """A seeded orthonormal axis (981 x 20) and variances in [0.5, 2]."""
    rng = np.random.default_rng(26)
    q, _ = np.linalg.qr(rng.standard_normal((981, D)))
    return q.astype(np.float32), rng.uniform(0.5, 2.0, D).astype(np.float32)


@pytest.fixture(scope="module")
def ref981(clouds, compress):
    p = pd_.packed(clouds, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM, 981)
    return p, pco.train(p.rows, compress[0], compress[1], rotate=True, exact=True)


def close(C, C_r, what):
    scale = np.abs(C_r).max()
    err = np.abs(C - C_r).max() / scale
    print("%s: correlation differs by %.2e of its largest entry" % (what, err))
    assert err <= BOUND, (what, err)


def solved(pca):
    pca.solve()
    return pca.nsample, pca.correlation()


def test_117_against_the_oracle(hctx, clouds, packed117, ref117):
    hctx.set_batch(64)
    pca = c3hlac.PCA(False)
    added, info = pca.add_c3_frames(hctx, clouds, rd.LEAF, 117, THR, **ARGS)
    assert added == N == packed117.n and (info["status"] == 0).all()
    n, C = solved(pca)
    assert n == N == ref117[3]
    close(C, ref117[4], "117")
    pca.close()


def test_981_compressed_rotate24_against_the_oracle(hctx, clouds, compress, ref981):
    hctx.set_batch(64)
    p, ref = ref981
    pca = c3hlac.PCA(False)
    pca.set_compress(compress[0], compress[1], D)
    added, info = pca.add_c3_frames(hctx, clouds, rd.LEAF, 981, THR, rotate24=True, **ARGS)
    assert added == N == p.n
    n, C = solved(pca)
    assert n == 24 * N == ref[3] and C.shape == (D, D)
    close(C, ref[4], "981 compressed, 24 rotations")
    # the same through the packed tensor and add_data
    out = hctx.extract_c3_frames_packed(clouds, rd.LEAF, 981, THR, **ARGS)[0]
    q = c3hlac.PCA(False)
    q.set_compress(compress[0], compress[1], D)
    q.add_data(out, rotate24=True)
    n2, C2 = solved(q)
    assert n2 == n
    close(C, C2, "add_c3_frames | packed + add_data")
    pca.close()
    q.close()


def test_batch_sizes_and_add_data_agree(hctx, clouds, ref117):
    got = []
    try:
        for b in (5, 64):
            hctx.set_batch(b)
            pca = c3hlac.PCA(False)
            added, _ = pca.add_c3_frames(hctx, clouds, rd.LEAF, 117, THR, **ARGS)
            assert added == N
            got.append(solved(pca))
            pca.close()
    finally:
        hctx.set_batch(64)
    assert got[0][0] == got[1][0] == N
    close(got[0][1], got[1][1], "set_batch(5) | set_batch(64)")
    close(got[0][1], ref117[4], "set_batch(5)")
    out = hctx.extract_c3_frames_packed(clouds, rd.LEAF, 117, THR, **ARGS)[0]
    q = c3hlac.PCA(False)
    q.add_data(out)
    close(got[1][1], solved(q)[1], "add_c3_frames | packed + add_data")
    q.close()


def test_streams_of_their_own_and_two_calls(clouds, ref117):
    """The context and the PCA object each on a torch stream; the clouds in two calls (the second
    call's first batch waits for the first call's SYRK before it writes the row buffer again)."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with c3hlac.Context(0) as c:
        c.set_stream(s1.cuda_stream)
        c.set_batch(7)
        pca = c3hlac.PCA(False)
        pca.set_stream(s2.cuda_stream)
        a1, _ = pca.add_c3_frames(c, clouds[:40], rd.LEAF, 117, THR, **ARGS)
        a2, _ = pca.add_c3_frames(c, clouds[40:], rd.LEAF, 117, THR, **ARGS)
        assert a1 + a2 == N
        n, C = solved(pca)
        assert n == N
        close(C, ref117[4], "own streams, two calls")
        pca.close()
        c.synchronize()
        c.set_stream(None)


def test_errors(hctx, clouds):
    hctx.set_batch(64)
    few = clouds[:3]
    pca = c3hlac.PCA(False)
    with pytest.raises(_capi.C3HError, match="improper dimension"):
        pca.add_c3_frames(hctx, few, rd.LEAF, 117, THR, rotate24=True, **ARGS)
    with pytest.raises(_capi.C3HError, match="C3H_ERR_ARG"):
        pca.add_c3_frames(hctx, few, rd.LEAF, 137, THR, **ARGS)
    added, info = pca.add_c3_frames(hctx, few + [sd.no_point()], rd.LEAF, 117, THR, **ARGS)
    assert info["status"].tolist() == [0, 0, 0, -3]
    with pytest.raises(_capi.C3HError, match="vector size differs"):
        pca.add_c3_frames(hctx, few, rd.LEAF, 981, THR, **ARGS)
    pca.solve()
    assert pca.nsample == added  # the refused calls added nothing
    # a negative threshold: every frame silent-empty, nothing added
    q = c3hlac.PCA(False)
    added0, info0 = q.add_c3_frames(hctx, few, rd.LEAF, 117, (147, -1, 148), **ARGS)
    assert added0 == 0 and (info0["status"] == 0).all()
    with pytest.raises(_capi.C3HError, match="no data"):
        q.solve()
    pca.close()
    q.close()
