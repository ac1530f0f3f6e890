"""Point clouds for the normals / RSD / GRSD edge-case tests (test_grsd_oracle_cpu.py,
test_gpu_grsd_edges.py).  Plain functions, no GPU.

edge_cloud: three surfaces (a tilted noisy plane that straddles z = 1, a noisy sphere, a
cylinder) so that every get_type class occurs, plus what the reference's shape clouds
never contain: isolated points (1 neighbour: NaN normal), a pair (2: NaN), a collinear
triple (degenerate covariance: the two smallest eigenvalues coincide), a right-angle
triple (exactly 3 neighbours, a well-defined normal), duplicate points and non-finite
rows inside the array."""
import numpy as np

SPHERE_C = (0.05, 0.05, 0.95)
N_PLANE, N_SPHERE, N_CYL = 1400, 1400, 900
LINE_DIR = np.array([1.0, 2.0, 2.0]) / 3.0  # direction of the collinear triple

# stragglers: every group at least 0.05 from the surfaces and from each other
SINGLES = [(0.0, -0.2, 0.9), (-0.2, -0.2, 1.05), (0.3, 0.1, 0.85)]
PAIR0 = (0.15, -0.1, 0.8)       # and 0.004 along x
LINE0 = (-0.1, -0.15, 0.9)      # and 0.005, 0.010 along LINE_DIR
CORNER0 = (0.15, 0.2, 0.9)      # and 0.005 along x, 0.005 along y


def edge_parts(seed=5):
    """The finite parts of edge_cloud, in order, as float64 (n_i, 3) arrays by name."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.08, 0.08, (2, N_PLANE))
    plane = np.stack([u + 0.30, v - 0.20, 1.0 + 0.3 * u - 0.2 * v + rng.normal(0, 0.0008, N_PLANE)], 1)
    d = rng.normal(size=(N_SPHERE, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = np.asarray(SPHERE_C) + 0.05 * d + rng.normal(0, 0.0005, (N_SPHERE, 3))
    th = rng.uniform(0, 2 * np.pi, N_CYL)
    cyl = np.stack([-0.2 + 0.03 * np.cos(th), rng.uniform(0.04, 0.16, N_CYL), 0.9 + 0.03 * np.sin(th)], 1)
    singles = np.array(SINGLES)
    pair = np.array(PAIR0) + np.array([[0, 0, 0], [0.004, 0, 0]])
    line = np.array(LINE0) + 0.005 * np.arange(3)[:, None] * LINE_DIR
    corner = np.array(CORNER0) + np.array([[0, 0, 0], [0.005, 0, 0], [0, 0.005, 0]])
    return dict(plane=plane, sphere=sphere, cylinder=cyl, singles=singles, pair=pair, line=line, corner=corner,
                dup=plane[:4].copy()), rng


def edge_cloud(seed=5, with_index=False):
    """(n, 4) float32 x y z rgb.  with_index: also {part name: row indices in the cloud}
    (and 'nonfinite')."""
    parts, rng = edge_parts(seed)
    xyz = np.concatenate(list(parts.values())).astype(np.float32)
    tag = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts.values())])
    bad = np.array([[np.nan, 0.1, 0.9], [0.1, 0.1, np.inf], [0.1, -np.inf, 0.9]], np.float32)
    xyz = np.insert(xyz, 100, bad[:1], axis=0)
    tag = np.insert(tag, 100, -1)
    xyz = np.insert(xyz, [2000, 2000], bad[1:], axis=0)
    tag = np.insert(tag, [2000, 2000], -1)
    rgb = rng.integers(0, 1 << 24, len(xyz)).astype(np.uint32).view(np.float32)
    pts = np.ascontiguousarray(np.concatenate([xyz, rgb[:, None]], 1), np.float32)
    if not with_index:
        return pts
    index = {name: np.flatnonzero(tag == k) for k, name in enumerate(parts)}
    index["nonfinite"] = np.flatnonzero(tag == -1)
    return pts, index


def big_plane(n=2 ** 21 + 1000, seed=9):
    """A noisy plane over 3 m x 3 m at z = 1 (z noise 0.001): more points than one pass of
    the grid-stride kernels covers (8192 blocks x 256 threads = 2^21)."""
    rng = np.random.default_rng(seed)
    pts = np.empty((n, 4), np.float32)
    pts[:, :2] = rng.uniform(-1.5, 1.5, (n, 2))
    pts[:, 2] = 1.0 + rng.normal(0, 0.001, n)
    pts[:, 3] = rng.integers(0, 1 << 24, n).astype(np.uint32).view(np.float32)
    return pts


def big_cells(seed=10):
    """A noisy plane at z = 1.01 (one layer of 0.02 cells) for a batch: 270 x 270 cells of 0.02 at
    about 28.8 points each (more than 65536 of them hold 16 points and more: one wave per such cell
    exceeds the cell-staged launch's 65536 workgroups), and a strip of five rows of cells at the
    largest y at about 4 points per cell, which sorts last and holds every sorted position from
    2^21 on (8192 x 256 threads cover 2^21 in their first pass)."""
    rng = np.random.default_rng(seed)
    nd, ns = 2 ** 21 - 100, 270 * 5 * 4  # 28.8 points per dense cell; the strip's 5400 sort behind them
    pts = np.empty((nd + ns, 4), np.float32)
    pts[:nd, 0] = rng.uniform(0.0, 5.4, nd)
    pts[:nd, 1] = rng.uniform(0.0, 5.4, nd)
    pts[nd:, 0] = rng.uniform(0.0, 5.4, ns)
    pts[nd:, 1] = rng.uniform(5.401, 5.499, ns)
    pts[:, 2] = 1.01 + rng.normal(0, 0.001, nd + ns)
    pts[:, 3] = rng.integers(0, 1 << 24, nd + ns).astype(np.uint32).view(np.float32)
    order = rng.permutation(nd + ns)  # the strip's rows anywhere in the input
    return pts[order]


def near_threshold(radii):
    """Voxels with an RSD radius within 1e-4 of a get_type threshold (reference radii)."""
    radii = np.asarray(radii, np.float64)
    near = np.zeros(len(radii), bool)
    for t in (0.100, 0.175, 0.015, 0.050):
        near |= (np.abs(radii - t) < 1e-4).any(1)
    return near | (np.abs(radii[:, 1] - radii[:, 0] - 0.050) < 1e-4)


def eigengap(pts, radius):
    """Relative gap (w1 - w0) / trace of the neighbourhood covariance of every row (float64;
    NaN where the normal is undefined) and the neighbour counts: where the gap is tiny the
    smallest eigenvector is not determined, and a normal cannot be compared."""
    xyz = pts[:, :3].astype(np.float32)
    ok = np.isfinite(xyz).all(1)
    P = xyz[ok]
    gap = np.full(len(pts), np.nan)
    cnt = np.zeros(len(pts), np.int64)
    r2 = np.float32(radius) * np.float32(radius)
    for i in np.flatnonzero(ok):
        d = P - xyz[i]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
        nb = P[d2 < r2].astype(np.float64)
        cnt[i] = len(nb)
        if len(nb) < 3:
            continue
        c = nb - nb.mean(0)
        w = np.linalg.eigvalsh(c.T @ c / len(nb))
        gap[i] = (w[1] - w[0]) / w.sum() if w.sum() > 0 else 0.0
    return gap, cnt
