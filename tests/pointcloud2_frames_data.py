"""Inputs shared by test_pointcloud2_frames_cpu.py and test_gpu_pointcloud2_frames.py: seeded
160 x 120 Kinect-style scenes on a 32^3 canvas (19,200 points: more than one 16,384-point
accumulate block per frame, the last one partial), the sensor_msgs/PointCloud2 messages built
from them in every record layout the loader has a form for, and the search settings."""
import functools

import numpy as np

from c3hlac import synth
from conftest import THR  # noqa: F401

G, LEAF, S, BOX, EXIST = 32, 0.02, 6, (2, 2, 2), 20
VARIANT, D, M, R = 117, 24, 2, 6
W, H = 160, 120
N = W * H
SEEDS = range(4)

# (point_step, offsets of x y z rgb)
KINECT = (32, (0, 4, 8, 16))     # PCL PointXYZRGB: VEC16, two pieces
FLOAT4 = (16, (0, 4, 8, 12))     # the packed record itself: VEC16, one piece
DWORD = (20, (4, 8, 12, 16))     # 4-byte aligned: one load per field
ODD = (19, (1, 5, 9, 14))        # byte by byte
NO_RGB = (32, (0, 4, 8, -1))     # rgb absent: read as 0


@functools.lru_cache(maxsize=None)
def bases():
    return synth.random_bases(VARIANT, D, M, R, seed=41)


@functools.lru_cache(maxsize=None)
def scene(s):
    """Scene s: (19200, 4) float32 with the generator's NaN rays plus 10 % NaN holes; the two
    sentinel points (cells (0,0,0) and (31,31,31)) stay, so the grid is 32^3 at min_b 0."""
    pts = synth.kinect_scene(N, grid=G, leaf=LEAF, seed=synth.BASE_SEED + 1700 + s)[:N].copy()
    holes = np.random.default_rng(100 + s).random(N) < 0.1
    holes[:2] = False
    pts[holes, :3] = np.nan
    pts.setflags(write=False)
    return pts


def variant(base, k):
    """test_gpu_points._variant on the host: colours XOR-masked, x shifted by k whole cells."""
    pts = base.copy()
    pts[:, 3] = (pts[:, 3].view(np.uint32) ^ np.uint32((k * 0x2F1D37) & 0xFFFFFF)).view(np.float32)
    pts[:, 0] = (pts[:, 0].astype(np.float64) + k * LEAF).astype(np.float32)
    return pts


def message(pts, height, width, layout=KINECT, row_pad=0, big=False, fill=0xAB):
    """The PointCloud2 message of the (height * width, 4) float32 array pts, row-major: records
    of layout[0] bytes with the four FLOAT32 fields at layout[1], every other byte (record
    padding, row padding) = fill, the last row without its padding.  Returns (msg, expect):
    expect is the array c3h_pointcloud2_to_xyzrgb must make of it (rgb 0 when absent)."""
    step, offs = layout
    n = height * width
    assert pts.shape == (n, 4) and pts.dtype == np.float32
    words = np.ascontiguousarray(pts).view(np.uint32)
    rec = np.full((n, step), fill, np.uint8)
    for k, off in enumerate(offs):
        if off >= 0:
            rec[:, off:off + 4] = np.ascontiguousarray(words[:, k].astype(">u4" if big else "<u4")).view(np.uint8) \
                .reshape(n, 4)
    rs = width * step + row_pad
    if n:
        buf = np.full((height, rs), fill, np.uint8)
        buf[:, :width * step] = rec.reshape(height, width * step)
        data = buf.reshape(-1)[:(height - 1) * rs + width * step].copy()
    else:
        data = np.zeros(0, np.uint8)
    fields = {"x": offs[0], "y": offs[1], "z": offs[2]}
    if offs[3] >= 0:
        fields["rgb"] = offs[3]
    expect = pts.copy()
    if offs[3] < 0:
        expect[:, 3] = 0
    msg = dict(height=height, width=width, point_step=step, row_step=rs, is_bigendian=int(big), fields=fields,
               data=data)
    return msg, expect
