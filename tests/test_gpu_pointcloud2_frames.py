"""PointCloud2 batches (c3h_run_pointcloud2_frames): the batched voxeliser reads the messages'
records in place.  The yardstick in every case is run_point_frames on the float arrays the
messages were built from: detection records and the whole frame-info array equal with
np.array_equal.  32^3 canvases, 160 x 120 messages (19,200 points: two accumulate blocks per
frame, the second partial), C3-HLAC-117 with 6-voxel subdivisions, 2 models, box 2 x 2 x 2.

Record layouts: the Kinect / PCL PointXYZRGB record (step 32, rgb at 16, row padding: two
16-byte loads per point), the packed float4 record (one), step 20 (one load per field), step 19
with odd offsets and a big-endian Kinect message (byte by byte), rgb absent.  Routes: device
and host messages, two batches with a partial one, frames that leave the batch (all NaN,
beyond the canvas), the exact-centroid pass on a point on a cell face (the message is read a
second time), mixed sizes with an empty message, rank 4 with three models and removeOverlap,
set_pipeline(False), argument errors, and one frame against the float64 oracle."""
import numpy as np
import pytest

import c3hlac
import pointcloud2_frames_data as pd
import pyoracle as po
from c3hlac import synth
from conftest import THR

pytestmark = pytest.mark.gpu
RTOL = 1e-5  # the project's bar against the float64 oracle


@pytest.fixture()
def pctx(ctx):
    """The shared context with this file's search settings; the defaults put back afterwards."""
    axis_t, var, axis_q = pd.bases()
    ctx.search_setup(axis_t, var, axis_q)
    ctx.set_rank(1)
    ctx.set_batch(8)
    ctx.set_pipeline(True)
    ctx.set_remove_overlap(False)
    yield ctx
    ctx.set_remove_overlap(False)
    ctx.set_pipeline(True)
    ctx.set_rank(1)
    ctx.set_batch(32)


def _call(ctx, fn, frames, per_frame):
    import torch
    d_out = torch.zeros((len(frames), per_frame * 3), dtype=torch.int64, device="cuda:0")
    nm, info = fn(frames, pd.LEAF, (pd.G,) * 3, pd.VARIANT, THR, pd.S, pd.BOX, pd.EXIST, True, d_out)
    return nm, d_out.cpu().numpy().view(c3hlac.DET_DTYPE).reshape(len(frames), per_frame), info


def _device(msg):
    import torch
    return dict(msg, data=torch.from_numpy(msg["data"]).cuda())


def _check(ctx, built, on_dev=True, per_frame=2):
    """built: [(msg, expect)].  Messages against the yardstick; returns the messages' results."""
    import torch
    msgs = [_device(m) if on_dev else m for m, _ in built]
    arrays = [torch.from_numpy(e).cuda() for _, e in built]
    torch.cuda.synchronize()
    nm_y, rec_y, info_y = _call(ctx, ctx.run_point_frames, arrays, per_frame)
    nm, rec, info = _call(ctx, ctx.run_pointcloud2_frames, msgs, per_frame)
    assert nm == nm_y
    assert np.array_equal(info, info_y), (info, info_y)
    assert np.array_equal(rec, rec_y), np.flatnonzero((rec != rec_y).any(1))
    return rec, info


def _kinect12():
    """12 frames of the Kinect layout: frame k's x shifted by k cells, its colours XOR-masked."""
    return [pd.message(pd.variant(pd.scene(k % 4), k), pd.H, pd.W, pd.KINECT, row_pad=16) for k in range(12)]


def test_kinect_layout_two_batches(pctx):
    import torch
    built = _kinect12()
    # the messages say what they are meant to say: the single-frame converter returns the arrays
    msg, expect = built[5]
    out = c3hlac.pointcloud2_to_xyzrgb(_device(msg))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    rec, info = _check(pctx, built)  # batch 8: two batches, the second partial
    assert (info["status"] == 0).all(), info["status"]
    assert np.array_equal(info["min_b"][:, 0], np.arange(12)) and (info["div_b"] == pd.G).all()
    assert (rec["score"] > 0).all()
    assert len({r.tobytes() for r in rec}) == 12  # every frame has results of its own


@pytest.mark.parametrize("layout,height,width,pad,big", [
    (pd.FLOAT4, 1, pd.N, 0, False),       # the float4 record itself: one 16-byte load per point
    (pd.DWORD, pd.H, pd.W, 4, False),     # one load per field
    (pd.ODD, pd.H, pd.W, 0, False),       # byte by byte: odd offsets and step
    (pd.ODD, pd.H, pd.W, 3, False),       #   and odd rows
    (pd.KINECT, pd.H, pd.W, 16, True),    # byte by byte: big-endian
    (pd.NO_RGB, pd.H, pd.W, 16, False),   # rgb absent: colours read as 0
], ids=["float4", "dword", "bytes", "bytes-rowpad", "bigendian", "no-rgb"])
def test_record_layouts(pctx, layout, height, width, pad, big):
    built = [pd.message(pd.variant(pd.scene(k % 4), k), height, width, layout, row_pad=pad, big=big)
             for k in range(3)]
    if layout is pd.NO_RGB:
        assert not built[0][1][:, 3].any() and pd.scene(0)[:, 3].view(np.uint32).any()
    rec, info = _check(pctx, built)
    assert (info["status"] == 0).all() and (rec["score"] > 0).all()


def test_host_messages_equal_device_messages(pctx):
    built = _kinect12()[:10]  # two batches; every message staged at a 16-byte aligned offset
    rec_h, info_h = _check(pctx, built, on_dev=False)
    rec_d, info_d = _check(pctx, built, on_dev=True)
    assert np.array_equal(rec_h, rec_d) and np.array_equal(info_h, info_d)
    # a layout whose messages are no multiple of 16 bytes long
    built = [pd.message(pd.variant(pd.scene(k), k), pd.H, pd.W, pd.ODD, row_pad=3) for k in range(3)]
    _check(pctx, built, on_dev=False)


def test_statuses_in_one_batch(pctx):
    good = [pd.variant(pd.scene(k), k) for k in range(3)]
    nan = np.full((pd.N, 4), np.nan, np.float32)  # no valid point: status 1, fresh setRank lists
    far = good[0].copy()  # extent beyond the canvas: status 1
    fin = np.flatnonzero(np.isfinite(far[:, 0]))
    far[fin[5], :3] = far[fin[6], :3] + np.float32(40 * pd.LEAF)
    edge = good[1].copy()  # a point right on a cell face: its voxel is summed exactly in the batch
    k = np.flatnonzero(np.isfinite(edge[:, 0]))[7]
    edge[k, 0] = np.float32(np.floor(edge[k, 0] / np.float32(pd.LEAF)) * np.float32(pd.LEAF))
    built = [pd.message(p, pd.H, pd.W, pd.KINECT, row_pad=16) for p in good + [nan, far, edge]]
    rec, info = _check(pctx, built)
    assert list(info["status"]) == [0, 0, 0, 1, 1, 0], info["status"]
    assert (rec[3]["score"] == 0).all() and (rec[[0, 1, 2, 4, 5]]["score"] > 0).all()


def test_sizes_mixed_in_one_batch(pctx):
    s = pd.scene(2)
    built = [pd.message(s, pd.H, pd.W, pd.KINECT, row_pad=16),
             pd.message(np.ascontiguousarray(s[:80 * 60]), 60, 80, pd.KINECT, row_pad=16),
             pd.message(np.ascontiguousarray(s[:1000]), 1, 1000, pd.KINECT),
             pd.message(np.zeros((0, 4), np.float32), 0, pd.W, pd.KINECT, row_pad=16),
             pd.message(pd.variant(s, 3), pd.H, pd.W, pd.KINECT, row_pad=16)]
    rec, info = _check(pctx, built)
    assert info["n_valid"][3] == 0 and info["status"][3] == 1
    assert info["status"][0] == 0 and info["status"][4] == 0 and (rec[[0, 4]]["score"] > 0).all()
    _check(pctx, built, on_dev=False)


def test_rank4_three_models_remove_overlap(pctx):
    axis_t, var, axis_q = synth.random_bases(pd.VARIANT, pd.D, 3, pd.R, seed=43)
    pctx.search_setup(axis_t, var, axis_q)
    pctx.set_rank(4)
    pctx.set_remove_overlap(True)
    built = _kinect12()[:10]
    rec, info = _check(pctx, built, per_frame=12)
    assert (info["status"] == 0).all()
    assert (rec["score"].max(1) > 0).all()  # (removeOverlap may take a model's best away: another model's wins)
    pctx.set_remove_overlap(False)
    rec_plain, _ = _check(pctx, built, per_frame=12)
    assert not np.array_equal(rec_plain, rec)  # removeOverlap did remove something


def test_pipeline_off(pctx):
    built = _kinect12()[:5]
    rec_on, info_on = _check(pctx, built)
    pctx.set_pipeline(False)
    rec, info = _check(pctx, built)
    assert (info["status"] == 1).all()
    assert np.array_equal(rec, rec_on)
    assert np.array_equal(info["div_b"], info_on["div_b"]) and np.array_equal(info["n_occ"], info_on["n_occ"])


def test_argument_errors_leave_the_context_usable(pctx):
    built = _kinect12()[:2]
    msgs = [_device(m) for m, _ in built]
    bad = [msgs[0], dict(msgs[1], fields={"x": 0, "y": 4, "z": 30, "rgb": 16})]
    bad[0] = dict(bad[0], fields=bad[1]["fields"])
    with pytest.raises(c3hlac.C3HError, match="field x/y/z missing or outside point_step"):
        _call(pctx, pctx.run_pointcloud2_frames, bad, 2)
    _check(pctx, built)
    bad = [msgs[0], dict(msgs[1], row_step=pd.W * 32 - 16)]
    with pytest.raises(c3hlac.C3HError, match="row_step < width \\* point_step"):
        _call(pctx, pctx.run_pointcloud2_frames, bad, 2)
    _check(pctx, built)


def test_one_frame_against_the_oracle(pctx):
    built = _kinect12()[5:6]
    rec, info = _check(pctx, built)
    pts = built[0][1]
    axis_t, var, axis_q = pd.bases()
    g, layout, cloud = po.voxelize(pts, pd.LEAF)
    assert list(info["div_b"][0]) == list(g.div_b) and list(info["min_b"][0]) == list(g.min_b)
    assert info["n_valid"][0] == g.n_valid and info["n_occ"][0] == g.n_occ == len(cloud)
    fe, sb, _ = po.c3hlac(g, layout, cloud, pd.VARIANT, THR, pd.LEAF, pd.S, exact=True)
    L, _, sc = po.search(sb, fe, po.exist(fe), synth.whiten(axis_t, var), axis_q, pd.BOX, 1, pd.EXIST, dbl=True,
                         want_scores=True)
    for m in range(pd.M):
        best = L.records()[m][0][0]
        assert best > 0 and abs(float(rec[0, m]["score"]) - best) <= RTOL * best, (m, rec[0, m], best)
