"""ConVOSCH ([GRSD-20 | C3-HLAC-981]) without a GPU: the oracle alone on the clouds of
convosch_data.py and on the frames of vosch_frames_data.py at variant 981, so that the GPU
checks of test_gpu_convosch.py are not vacuous.  These are conditions on the inputs, not
tolerances."""
import numpy as np

import convosch_data as cd
import pyoracle as po
import vosch_frames_data as vd
from conftest import THR


def test_white_plane_sums_pass_32_bits():
    pts = cd.white_plane()
    g, layout, cloud = po.voxelize(pts, cd.LEAF)
    assert tuple(g.div_b[:3]) == (300, 300, 1) and g.n_occ == 90_000
    assert vd.moved_voxels(g, layout, cloud, cd.LEAF) == 0
    feat, sb, hn = po.c3hlac(g, layout, cloud, 981, cd.THR_MID, cd.LEAF, cd.PLANE_SUBDIV, exact=True)
    assert hn == 1 and feat.shape == (1, 981)
    raw = feat[0, 6:495].astype(np.float64) * 65025  # the second-order sums, to float32 rounding
    big = raw > 2.0 ** 32
    assert big.sum() == 42, big.sum()
    # the largest is bin 474, the auto-product of channel 0 over every voxel: the LUT takes 255 to
    # (254, 0), so 90,000 * 254^2 = 5,806,440,000 (the feature is that sum times float(1 / 65025))
    assert tuple(po.lut()[255]) == (254, 0)
    top = 90_000 * 254 * 254
    assert int(np.argmax(raw)) == 474 - 6 and abs(raw.max() - top) <= top * 2.0 ** -22


def test_dense_cube_rows():
    pts = cd.dense_cube()
    g, layout, cloud = po.voxelize(pts, cd.LEAF)
    assert tuple(g.div_b[:3]) == (12, 12, 12) and g.n_occ == 12 ** 3
    assert vd.moved_voxels(g, layout, cloud, cd.LEAF) == 0
    feat, sb, hn = po.c3hlac(g, layout, cloud, 981, cd.THR_MID, cd.LEAF, cd.CUBE_SUBDIV, exact=True)
    assert hn == 8 and tuple(sb) == (2, 2, 2)
    assert po.exist(feat).tolist() == cd.CUBE_EXIST
    assert (feat[0] != 0).all()  # 1,000 voxels with every neighbour present: no zero among the 981 bins


def test_frames_of_the_batch_at_variant_981():
    """What test_vosch_frames_cpu.py says of the frames holds for the 981 columns too: voxels
    whose centroid lies in another cell (1 and 14), frames without rows, a frame without a point."""
    d = dict(vd.batch())
    g, layout, cloud = po.voxelize(d["edge"], vd.LEAF)
    assert vd.moved_voxels(g, layout, cloud, vd.LEAF) == 1
    feat, sb, hn = po.c3hlac(g, layout, cloud, 981, THR, vd.LEAF, vd.SUBDIV, vd.OFFSET, exact=True)
    assert tuple(sb) == vd.subdivisions(g.div_b[:3]) and hn == int(np.prod(sb)) and hn > 1
    assert (po.exist(feat) > 0).sum() > 1
    g, layout, cloud = po.voxelize(d["bowl1_0000"], vd.FINE_LEAF)
    assert g.n_occ == 945 and vd.moved_voxels(g, layout, cloud, vd.FINE_LEAF) == 14
    feat, sb, hn = po.c3hlac(g, layout, cloud, 981, THR, vd.FINE_LEAF, vd.SUBDIV, vd.OFFSET, exact=True)
    assert hn == int(np.prod(vd.subdivisions(g.div_b[:3]))) and (po.exist(feat) > 0).any()
    for name in ("noisy_plane_purple", "noisy_torus_blue"):  # thinner than the z offset: no row
        g, layout, cloud = po.voxelize(d[name], vd.LEAF)
        assert vd.subdivisions(g.div_b[:3]) == (0, 0, 0)
        assert po.c3hlac(g, layout, cloud, 981, THR, vd.LEAF, vd.SUBDIV, vd.OFFSET, exact=True)[2] <= 0
    assert len(d["no_point"]) == 0
