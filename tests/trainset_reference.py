"""The device-resident training set restated in NumPy float64 and Python integers (what csrc/trainset_device.hpp,
vpk_trainset_batch, train.TrainSet and train.Solver are held to).  The four formulas are written with element-wise array
operations, which round every product, sum and difference on its own."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ---- counter-based draws --------------------------------------------------------------------------------------------------
def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def mask_key(seed, iteration, layer, b):
    h0 = mix64((seed + GOLDEN * (iteration + 1)) & M64)
    return mix64(h0 ^ ((layer << 32) | b))


def draw(seed, iteration, b, k):
    """u_k of slot b: an integer below 2^53 times 2^-53, exact in float64"""
    return float(mix64(mask_key(seed, iteration, 0x41, b) ^ k) >> 11) * 2.0 ** -53


def order(seed, epoch, n, shuffle):
    if not shuffle:
        return list(range(n))
    k0 = mask_key(seed, epoch, 0x53, 0)
    return sorted(range(n), key=lambda i: (mix64(k0 ^ i), i))


def indices(iteration, batch, n, seed, shuffle):
    out = []
    for b in range(batch):
        p = iteration * batch + b
        out.append(order(seed, p // n, n, shuffle)[p % n])
    return out


def augment_transforms(seed, iteration, batch, max_rotation, max_scale, max_shift, mirror):
    """H = T(tx, ty) . S(s) . R(theta) . diag(m, 1, 1) as matrix products (every sum adds exact zeros only)"""
    out = np.zeros((batch, 6))
    for b in range(batch):
        u = [draw(seed, iteration, b, k) for k in range(5)]
        theta = (2 * u[0] - 1) * max_rotation
        m = -1.0 if u[1] < mirror else 1.0
        s = np.exp((2 * u[2] - 1) * np.log(max_scale))
        tx, ty = (2 * u[3] - 1) * max_shift, (2 * u[4] - 1) * max_shift
        T = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        S = np.diag([s, s, 1.0])
        R = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1.0]])
        H = T.dot(S).dot(R).dot(np.diag([m, 1.0, 1.0]))
        out[b] = H[:2].ravel()
    return out


# ---- the four formulas -------------------------------------------------------------------------------------------------------
def transform_lines(h, l):
    """h (6,) or (n, 6); l (n, 3) -> det * H^-T l"""
    h = np.asarray(h, dtype=np.float64).reshape(-1, 6)
    l = np.asarray(l, dtype=np.float64).reshape(-1, 3)
    h00, h01, h02, h10, h11, h12 = (h[:, i] for i in range(6))
    lx, ly, lz = l[:, 0], l[:, 1], l[:, 2]
    det = h00 * h11 - h01 * h10
    mx = h11 * lx - h10 * ly
    my = h00 * ly - h01 * lx
    mz = det * lz - (h02 * mx + h12 * my)
    return np.stack([mx, my, mz], 1)


def transform_vps(h, v):
    h = np.asarray(h, dtype=np.float64).reshape(-1, 6)
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    h00, h01, h02, h10, h11, h12 = (h[:, i] for i in range(6))
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    wx = (h00 * vx + h01 * vy) + h02 * vz
    wy = (h10 * vx + h11 * vy) + h12 * vz
    return np.stack([wx, wy, vz * np.ones_like(wx)], 1)


# ---- labels ------------------------------------------------------------------------------------------------------------------
def fractional_index(vps, grid):
    """label_maps' fractional cell index of every VP (NaN rows for VPs it drops before the index)"""
    from vanishing_points_2017_amd import coordinate_conversion as cc
    vps = np.asarray(vps, dtype=np.float64).reshape(-1, 3)
    out = np.full((vps.shape[0], 2), np.nan)
    with np.errstate(all="ignore"):
        for i, row in enumerate(vps):
            norm = np.sqrt(np.sum(row * row))
            if not norm > 0 or not np.all(np.isfinite(row)):
                continue
            p = row / norm
            if p[2] < 0:
                p = -p
            out[i] = cc.angle_to_index(cc.point_to_angle(p), grid)
    return out


def cells(vps, grid):
    """the cell a * gw + b of every VP through train.label_maps itself, -1 where it sets nothing"""
    from vanishing_points_2017_amd import train
    vps = np.asarray(vps, dtype=np.float64).reshape(-1, 3)
    out = np.full(vps.shape[0], -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i, row in enumerate(vps):
            hit = np.flatnonzero(train.label_maps(row[None], grid).ravel())
            assert hit.size <= 1
            if hit.size:
                out[i] = hit[0]
    return out


def margin(vps, grid):
    """the smallest distance of a finite fractional index to a k + 0.5 (the rounding boundary of floor(idx + 0.5))"""
    idx = fractional_index(vps, grid)
    idx = idx[np.isfinite(idx)]
    if idx.size == 0:
        return np.inf
    frac = idx - np.floor(idx)
    return float(np.abs(frac - 0.5).min())


def batch(lines, vps, index, transforms, grid):
    """what vpk_trainset_batch gives for the examples ``index``: l_out, vp_out, cell_out, labels (B, gh * gw), offsets"""
    from vanishing_points_2017_amd import train
    l_out, vp_out, labels, counts = [], [], [], []
    for b, i in enumerate(index):
        l = np.asarray(lines[i], dtype=np.float64).reshape(-1, 3)
        v = np.asarray(vps[i], dtype=np.float64).reshape(-1, 3)
        if transforms is not None:
            l = transform_lines(transforms[b], l) if l.shape[0] else l
            v = transform_vps(transforms[b], v) if v.shape[0] else v
        l_out.append(l)
        vp_out.append(v)
        counts.append(l.shape[0])
        with np.errstate(all="ignore"):
            labels.append(train.label_maps(v, grid).ravel())
    vp_cat = np.concatenate(vp_out, 0)
    off = np.zeros(len(index) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    return {"l_out": np.concatenate(l_out, 0), "vp_out": vp_cat, "cell_out": cells(vp_cat, grid),
            "labels": np.stack(labels).astype(np.float32), "offsets": off, "lines": l_out}


# ---- the solver's schedule -----------------------------------------------------------------------------------------------------
def schedule(max_iter, test_interval, display, snapshot, start=0):
    """Caffe's Solver::Step / Solve as a list of (event, iteration): a test before the iteration's step where the iteration
    is a multiple of test_interval, the display of that step's loss, a snapshot once the count of finished iterations is a
    multiple of ``snapshot``, one at the end unless just taken, a last test if max_iter is a multiple of test_interval"""
    ev = []
    it = start
    last = None
    while it < max_iter:
        if test_interval and it % test_interval == 0:
            ev.append(("test", it))
        if display and it % display == 0:
            ev.append(("display", it))
        it += 1
        if snapshot and it % snapshot == 0:
            ev.append(("snapshot", it))
            last = it
    if last != it:
        ev.append(("snapshot", it))
    if test_interval and it % test_interval == 0:
        ev.append(("test", it))
    return ev


# ---- the ten-image set of the tests ------------------------------------------------------------------------------------------
EDGE_LINES = (0, 1, 63, 64, 65, 513, 2, 7, 130, 300)
EDGE_VPS = (0, 1, 3, 8, 2, 3, 3, 1, 4, 3)
EDGE_SEED = 1                 # admitted by tests/test_trainset.py::test_edge_set_margins: every VP of every case keeps its margin
EDGE_AUGMENT = (0.3, 1.25, 0.1, 0.5)
EDGE_ITERATIONS = (1, 6)
EDGE_BATCHES = (1, 5, 32)
EDGE_GRIDS = ((20, 20), (4, 4), (1, 1))
MARGIN = 1e-6


def edge_set(seed=EDGE_SEED):
    """(lines, vps): segments inside the normalised image as homogeneous lines; VPs as directions of the upper half sphere
    at assorted lengths.  Image 3 has two VPs in one cell, image 4 a VP given with z < 0, image 6 a zero VP."""
    rs = np.random.RandomState(seed)
    lines, vps = [], []
    for n, m in zip(EDGE_LINES, EDGE_VPS):
        p1 = np.concatenate([rs.uniform(-1, 1, (n, 2)), np.ones((n, 1))], 1)
        p2 = np.concatenate([rs.uniform(-1, 1, (n, 2)), np.ones((n, 1))], 1)
        lines.append(np.ascontiguousarray(np.cross(p1, p2)).reshape(-1, 3))
        v = rs.standard_normal((m, 3))
        v[:, 2] = np.abs(v[:, 2]) + 0.05
        vps.append(v * rs.uniform(0.5, 3.0, (m, 1)))
    vps[3][1] = vps[3][0] * 1.5 + np.array([1e-3, -1e-3, 0.0])
    vps[4][0] = -vps[4][0]
    vps[6][1] = 0.0
    return lines, vps


def edge_cases():
    """(batch, iteration or None for the identity) of the GPU comparison"""
    return [(b, it) for b in EDGE_BATCHES for it in (None,) + EDGE_ITERATIONS]
