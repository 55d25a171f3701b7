"""Deterministic scenes that take the device velocity estimator (dspmap_velest.hip) past its small-scene paths.

Every builder returns a Scene: sensor-frame clouds, one per frame, for the small map of the estimator tests (66 x 66 x 40 voxels of
0.15 m, filter resolution 0.1 m), seen from (0, 0, 1.0) with the identity attitude like tests/test_gpu_round2.py:_cluster_scene, plus
what the scene claims about itself (`expect`); tests/test_velest_cpu.py pins every claim with the oracle, on the CPU.

How the clouds are made
  * a cluster is a tight group of >= 5 points (0.1 m apart, or 0.195 m in `dense`); two clusters are never closer than 0.21 m, the
    tolerance being 2 * res_filter = 0.2 m;
  * the input order of every frame is a seeded permutation: the members of a cluster are spread over the slices of k_ve_components and
    the roots (smallest index of a component) are in no spatial order;
  * points that must be connected ONLY by pairs at exactly the tolerance use LINK: a vector on the 2^-21 grid whose squared length,
    summed the way the kernel and the oracle sum it (fp32, no contraction), equals fl(tol * tol) bit for bit.

Two things the arithmetic does not allow, stated here once:
  * with the sensor 1.0 m above the ground a world height near 0.1 is a multiple of 2^-24 (fl(z_s + 1) with z_s in (-1, -0.5)), and
    res_filter = 0.1f is not one.  The "ground at exactly res_filter" sheet therefore sits on the two neighbouring multiples: the
    largest one below 0.1f (ground) and the smallest one above it (not ground).  No closer pair exists at this height.
  * `dense` and the scaling tool's scenes past ~230 clusters do not fit into the part of the field of view that lies inside the
    9.9 m map (4 500 tolerance cells alone are 36 of its ~50 cubic metres): their points reach out to x = 7.6 m.  Points in view
    beyond the map are ordinary input (the birth stage drops their children on both sides); all other scenes stay inside the map.
"""
import functools

import numpy as np

F = np.float32
POS = (0.0, 0.0, 1.0)
QUAT = (1.0, 0.0, 0.0, 0.0)
DT = 0.1
CFG = dict(nx=66, ny=66, nz=40, res=0.15, ppv=9)
RES_F = F(0.1)
TOL = F(2) * RES_F
TOL2 = TOL * TOL
TAN_H, TAN_V = 0.85, 0.42      # inside tan(42 deg) = 0.900 and tan(24 deg) = 0.445
NRAND = 50021                  # common.tables' rand() table
GRID = 2.0 ** -21              # every value below 8 on this grid is an fp32 number, and so are sums / differences of two of them


def d2_f32(a, b):
    """squared distance as the kernel and the oracle compute it: fp32, left to right, every operation rounded"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    e = (a - b).astype(F)
    return F(F(F(e[..., 0] * e[..., 0]) + F(e[..., 1] * e[..., 1])) + F(e[..., 2] * e[..., 2]))


def world(pts):
    """sensor frame -> world as :1389-1391 does it (fp32 add of the position)"""
    return (np.asarray(pts, F) + np.asarray(POS, F)).astype(F)


def q(v):
    return np.round(np.asarray(v, np.float64) / GRID) * GRID


@functools.lru_cache(None)
def link():
    """(lx, ly, lz) near (0.0866, 0.1, 0.15) on the 2^-21 grid with fl(fl(lx^2 + ly^2) + lz^2) == fl(tol^2) in fp32"""
    ly, lz0 = q(0.1), q(0.15)
    for dz in range(0, 400):
        for dx in range(-400, 400):
            lx, lz = q(0.0866) + dx * GRID, lz0 + dz * GRID
            v = np.array([lx, ly, lz], F)
            if d2_f32(v, np.zeros(3, F)) == TOL2:
                return float(lx), float(ly), float(lz)
    raise AssertionError("no exact link")


class Scene:
    def __init__(self, name, frames, expect, r_cursor=None):
        self.name, self.frames, self.expect, self.r_cursor = name, frames, expect, r_cursor
        self.pos, self.quat, self.dt = POS, QUAT, DT

    def stamp(self, f):
        return f * DT


def _shuffle(parts, seed):
    pts = np.concatenate(parts).astype(F)
    return pts[np.random.default_rng(seed).permutation(len(pts))]


def _sheet(x, y0, z0, n, nz, step=0.1):
    """n points of a y-z sheet at depth x, filled column by column (nz points per column): connected for every n"""
    i = np.arange(n)
    return np.stack([np.full(n, x), y0 + step * (i // nz), z0 + step * (i % nz)], 1)


STICKS = [(1, 5), (1, 6), (2, 5), (2, 6), (1, 5), (2, 5), (1, 6)]   # (ny, nz): 5, 6, 10, 12 points, many equal sizes


class _Lattice:
    """slots for small clusters: rows of constant depth x = 1.5 + 0.3 r, 0.4 m apart in y, two tiers in z (z_s from -0.6 and from
    0.15).  A row moves as a whole (dy_r per step), so the 0.3 m gaps inside a row stay; rows are 0.3 m apart in x."""
    def __init__(self, rows, seed, lo_rows=None):
        self.slots = []
        for r in range(rows):
            x = 1.5 + 0.3 * r
            n = int((2 * TAN_H * x - 0.05 - 0.1 - 0.3) / 0.4) + 1
            for tier in ("lo", "hi"):
                if tier == "hi" and TAN_V * x < 0.15 + 0.5 + 0.04:
                    continue
                if tier == "lo" and lo_rows is not None and r >= lo_rows:
                    continue
                self.slots += [(r, tier, i) for i in range(n)]
        order = np.random.default_rng(seed).permutation(len(self.slots))
        self.slots = [self.slots[k] for k in order]
        self.taken = set()

    def take(self, slot=None):
        if slot is None:
            slot = next(s for s in self.slots if s not in self.taken)
        assert slot not in self.taken
        self.taken.add(slot)
        return slot

    @staticmethod
    def row_dy(r):
        return 0.03 + 0.005 * r

    @staticmethod
    def stick(slot, shape, j, step, z0=None, jitter=True):
        """the points of stick j in its slot after `step` moves"""
        r, tier, i = slot
        x = 1.5 + 0.3 * r
        ny, nz = shape
        y0 = -TAN_H * x + 0.05 + 0.4 * i + step * _Lattice.row_dy(r)
        zb = (-0.6 if tier == "lo" else 0.15) if z0 is None else z0
        zb += step * 0.005 * (j % 5) if jitter else 0.0
        ys, zs = np.meshgrid(y0 + 0.1 * np.arange(ny), zb + 0.1 * np.arange(nz), indexing="ij")
        return np.stack([np.full(ys.size, x), ys.ravel(), zs.ravel()], 1)


def _ground_straddle():
    """sensor heights z_lo < z_hi, neighbours on the 2^-24 grid, with fl(z_lo + 1) <= res_filter < fl(z_hi + 1)"""
    z = F(-0.9)
    while F(z + F(1.0)) > RES_F:
        z = np.nextafter(z, F(-2))
    while F(np.nextafter(z, F(0)) + F(1.0)) <= RES_F:
        z = np.nextafter(z, F(0))
    return z, np.nextafter(z, F(0))


def _ground_sheet():
    """12 x 32 points, 0.1 m apart: most at the largest world height <= res_filter (ground), some one float higher (NOT ground: isolated
    points 0.3 x 0.4 m apart and one group of four -- all below the minimum cluster size, so the birth cloud drops them).
    Returns (points, number of dropped points)"""
    z_lo, z_hi = _ground_straddle()
    ix, iy = np.meshgrid(np.arange(12), np.arange(32), indexing="ij")
    above = ((ix % 3 == 0) & (iy % 4 == 0) & (iy >= 8)) | ((ix >= 5) & (ix <= 6) & (iy >= 2) & (iy <= 3))
    ix, iy, above = ix.ravel(), iy.ravel(), above.ravel()
    pts = np.stack([2.3 + 0.1 * ix, -1.6 + 0.1 * iy, np.zeros(ix.size)], 1).astype(F)
    pts[:, 2] = np.where(above, z_hi, z_lo)
    return pts, int(above.sum())


def _chain(x0, y0, zw0, n=6):
    """n points, consecutive ones exactly the tolerance apart (LINK), no other pair within it: a zigzag rising in z"""
    lx, ly, lz = link()
    k = np.arange(n)
    p = np.stack([q(x0) + lx * (k % 2), q(y0) + ly * (k % 2), q(zw0) + lz * k - 1.0], 1)
    return p


def k_edge(K, name=None, r_cursor=None):
    """K clusters in every one of three frames: sticks of 5 / 6 / 10 / 12 points, sheets of 64, 65, 128, 129,
    192, 193, 200 and 201 (static by size) points, one stick whose centre is just above 1.5 m (static) and one just below, a 6-point
    chain at exactly the tolerance, a sheet that grows from 20 to 130 points in frame 1 (gated by size), one that has 150 / 210 / 150
    points (possibly dynamic, static, possibly dynamic: the matching is K-3 x K-2, then K-2 x K-3), a stick that moves 0.55 m per frame
    (> 5 m/s: velocity zeroed), and the ground sheet around res_filter.  Frame 1: every row of the lattice moves 0.03 .. 0.085 m in y and
    the sticks up to 0.02 m in z.  Frame 2: a third of the clusters (sticks) are gone and as many new ones stand in other slots."""
    assert K >= 40
    lat = _Lattice(12, seed=K, lo_rows=8)
    chain_slot = (5, "lo", 9)
    lat.take(chain_slot); lat.take((5, "hi", 9))
    hi_slot, lo_slot = lat.take((3, "hi", 2)), lat.take((3, "hi", 6))
    n_sticks = K - 14
    n_swap = K // 3
    sticks = [(lat.take(), STICKS[j % len(STICKS)], j) for j in range(n_sticks + n_swap)]
    ground, n_drop = _ground_sheet()
    sizes_big = {11: (200, 201, 64), 10: (192, 193, 65), 9: (128, 129, None)}
    frames, chains = [], []
    for f in range(3):
        parts = [ground]
        for r, row in sizes_big.items():
            x = 1.5 + 0.3 * r
            y = -TAN_H * x + 0.05 + f * _Lattice.row_dy(r)
            for n in row:
                room = 130 if n is None else n
                if n is None:
                    n = 20 if f == 0 else 130      # |dn| = 110 > 100: the gate closes, the cluster stays unmatched in frame 1
                parts.append(_sheet(x, y + (0.7 if n == 20 else 0.0), -0.8, n, 8))   # (the 20 points: the middle of the 130)
                y += 0.1 * ((room + 7) // 8 - 1) + 0.3
        x = 1.5 + 0.3 * 8
        y = -TAN_H * x + 0.05 + f * _Lattice.row_dy(8)
        parts.append(_sheet(x, y, -0.8, 210 if f == 1 else 150, 8))
        parts.append(_sheet(x, y + 3.0 + f * 0.55, -0.6, 12, 6))                                        # the fast one
        parts.append(_Lattice.stick(hi_slot, (1, 5), 0, f, z0=0.304, jitter=False))                    # centre at 1.504 m: static
        parts.append(_Lattice.stick(lo_slot, (1, 5), 0, f, z0=0.296, jitter=False))                    # centre at 1.496 m
        xs = 1.5 + 0.3 * chain_slot[0]
        chains.append(_chain(xs, -TAN_H * xs + 0.05 + 0.4 * chain_slot[2] + f * 0.0625, 0.4))
        parts.append(chains[-1])
        live = range(n_sticks) if f < 2 else range(n_swap, n_sticks + n_swap)
        for k in live:
            slot, shape, j = sticks[k]
            parts.append(_Lattice.stick(slot, shape, j, f))
        frames.append(_shuffle(parts, 1000 * K + f))
    expect = dict(K=[K] * 3, n_dyn=[K - 2, K - 3, K - 2], dropped=[n_drop] * 3, outside=[0] * 3,
                  sizes={64, 65, 128, 129, 192, 193, 200, 201, 5, 6, 10, 12},
                  hungarian=[None, (K - 3, K - 2), (K - 2, K - 3)], steps=[None, "N..T", "N..T"], in_map=True,
                  chains=chains, ground_above=n_drop, ground_points=len(ground))
    return Scene(name or "k_edge_%d" % K, frames, expect, r_cursor)


def rand_wrap():
    """k_edge(65) with the rand() cursor 20 draws before the end of the table: the 65 intensity draws of frame 0 wrap it"""
    return k_edge(65, name="rand_wrap", r_cursor=NRAND - 20)


HUNGARIAN_EDGE_NDYN = [64, 64, 65, 65, 64, 130, 70, 130]


def benign(n_dyn_per_frame, name, rows=12, seed=7):
    """sticks only (all possibly dynamic) plus one static sheet of 201 points; frame f shows the first n_dyn[f] sticks of a fixed
    shuffled list; odd frames are moved by one step of the lattice (0.03 .. 0.13 m): real-valued costs between neighbours, gated ones
    between clusters 1.5 m or more apart"""
    lat = _Lattice(rows, seed=seed, lo_rows=rows - 1)
    sticks = [(lat.take(), STICKS[j % len(STICKS)], j) for j in range(max(n_dyn_per_frame))]
    r = rows - 1
    x = 1.5 + 0.3 * r
    frames = []
    for f, n in enumerate(n_dyn_per_frame):
        parts = [_sheet(x, -TAN_H * x + 0.05 + (f % 2) * _Lattice.row_dy(r), -0.8, 201, 8)]
        parts += [_Lattice.stick(slot, shape, j, f % 2) for slot, shape, j in sticks[:n]]
        frames.append(_shuffle(parts, 77000 + 100 * seed + f))
    nd = list(n_dyn_per_frame)
    expect = dict(K=[n + 1 for n in nd], n_dyn=nd, dropped=[0] * len(nd), outside=[0] * len(nd), sizes={201, 5, 6, 10, 12},
                  hungarian=[None] + [(nd[f], nd[f - 1]) for f in range(1, len(nd))], steps=[None] + ["N..T"] * (len(nd) - 1),
                  in_map=rows <= 12)
    return Scene(name, frames, expect)


def hungarian_edge():
    """(n_dyn, n_last) = (64, 64), (65, 64), (65, 65), (64, 65), (130, 64), (70, 130), (130, 70): both sides of N = 64 with square and
    rectangular problems in both directions, by changing the number of clusters between frames"""
    return benign(HUNGARIAN_EDGE_NDYN, "hungarian_edge")


CORNERS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float64) * 0.1


def all_gated(K, name=None):
    """K clusters of 5 .. 8 points (corners of a 0.1 m cube) on a 0.31 m lattice in a slab that is thin in x; frame 1 shows the same
    clusters moved along x by the slab's thickness + 1.59 m or more (2.0 m up to K = 130): EVERY pair of a new and an old cluster is
    1.5 m or more apart, every cost is the gate's 7 500, the matrix is all-equal: N (N + 1) / 2 steps of the matching, no velocity"""
    if K <= 130:
        x0, ny, layers = 2.3, 13, 2
    else:
        x0, ny = 4.4, 24
        layers = -(-K // (ny * 5))
    move = 2.0 if K <= 130 else 0.31 * (layers - 1) + 0.1 + 1.6
    assert x0 + 0.31 * (layers - 1) + 0.1 + move < 7.6
    cl = []
    for k in range(K):
        ix, rest = divmod(k, ny * 5)
        iz, iy = divmod(rest, ny)
        org = np.array([x0 + 0.31 * ix, -0.31 * (ny - 1) / 2 - 0.05 + 0.31 * iy, -0.88 + 0.31 * iz])
        cl.append(org + CORNERS[:5 + k % 4])
    frames = [_shuffle([c + np.array([f * move, 0, 0]) for c in cl], 88000 + K + f) for f in range(2)]
    expect = dict(K=[K] * 2, n_dyn=[K] * 2, dropped=[0] * 2, outside=[0] * 2, sizes={5, 6, 7, 8},
                  hungarian=[None, (K, K)], steps=[None, "T"], in_map=K <= 130)
    return Scene(name or "all_gated_%d" % K, frames, expect)


def _snake(x, y0, zw0, m, segs, sign=1):
    """`segs` runs of m points along y (0.1 m apart, 0.3 m above one another), joined end to end by ONE bridge point each that is exactly
    the tolerance from the end of one run and from the start of the next (LINK); nothing else connects two runs"""
    lx, ly, lz = link()
    out = []
    y_end = q(y0)
    for s in range(segs):
        d = sign * (1 if s % 2 == 0 else -1)
        ys = y_end + d * q(0.1) * np.arange(m)
        zw = q(zw0) + 2 * lz * s
        out.append(np.stack([np.full(m, q(x)), ys, np.full(m, zw - 1.0)], 1))
        y_end = ys[-1]
        if s + 1 < segs:
            out.append(np.array([[q(x) + lx, y_end + d * ly, zw + lz - 1.0]]))
    return np.concatenate(out)


DENSE_SHAPES = [(2, 3), (3, 3), (2, 4), (3, 4), (4, 4), (3, 2), (4, 3), (4, 2)]


def dense():
    """exactly 6 144 input points, 400 of them outside the field of view; more than 300 clusters of 6 .. 16 points 0.195 m apart (nearly
    one tolerance cell per point: far more occupied cells than the 4 096 buckets), four snakes of 151 .. 199 points, five groups below
    the minimum size, ground for the rest.  Frames move everything by 0.02 m in y."""
    s = 0.195
    pitch = 3 * s + 0.21
    fixed = []       # snakes + small groups (sensor frame)
    snakes = [(5.0, -1.9, 0.2, 39, 4), (5.0, -1.9, 1.5, 39, 5), (5.6, 1.8, 0.2, 37, 4), (5.6, 2.25, 1.5, 46, 4)]
    for x, y0, zw0, m, segs in snakes:
        fixed.append(_snake(x, y0, zw0, m, segs, sign=1 if y0 < 0 else -1))
    small = [np.stack([np.full(n, 1.09), np.full(n, -0.9 + 0.45 * g), 0.1 * np.arange(n)], 1) for g, n in enumerate([1, 2, 3, 4, 1])]
    n_small = sum(len(p) for p in small)
    n_out, n_ground_min = 400, 60
    budget = 6144 - n_out - sum(len(p) for p in fixed) - n_small - n_ground_min
    xs = []
    x = 1.3
    while x < 7.55:
        if abs(x - 5.0) < 0.35 or abs(x - 5.6) < 0.35:      # the snakes' layers (their bridges stand 0.087 m in front)
            x += 0.21
            continue
        xs.append(x)
        x += 0.21
    tiles = []
    for band in (0, 1):                                       # low tiles first: most clusters stay below 1.5 m
        for x in xs:
            z_lo, z_hi = max(-TAN_V * x, -0.85), min(TAN_V * x, 2.8)
            nzt = int((z_hi - z_lo - 3 * s) / pitch) + 1
            nyt = int((2 * TAN_H * x - 0.06 - 3 * s) / pitch) + 1
            for iz in range(nzt):
                z0 = z_lo + pitch * iz
                if (z0 <= 0.3) != (band == 0):
                    continue
                tiles += [(x, -TAN_H * x + pitch * iy, z0) for iy in range(nyt)]
    clusters = []
    used = 0
    n_dyn = 2                                                 # the two low snakes
    for k, (x, y0, z0) in enumerate(tiles):
        a, b = DENSE_SHAPES[k % len(DENSE_SHAPES)]
        if used + a * b > budget:
            break
        n_dyn += 1 if 1.0 + z0 + s * (b - 1) / 2 <= 1.5 else 0
        ys, zs = np.meshgrid(y0 + s * np.arange(a), z0 + s * np.arange(b), indexing="ij")
        clusters.append(np.stack([np.full(a * b, x), ys.ravel(), zs.ravel()], 1))
        used += a * b
    n_ground = 6144 - n_out - sum(len(p) for p in fixed) - n_small - used
    g = np.arange(n_ground)
    ground = np.stack([2.5 + 0.1 * (g % 40), -1.0 + 0.1 * (g // 40), np.full(n_ground, -0.95)], 1)
    o = np.arange(n_out)
    outside = np.stack([-1.0 - 0.01 * o, 0.005 * o - 1.0, 0.3 * np.sin(o)], 1)       # behind the sensor
    frames = []
    for f in range(3):
        shift = np.array([0.0, float(q(0.02)) * f, 0.0])
        parts = [p + shift for p in fixed + small + clusters + [ground]] + [outside]
        frames.append(_shuffle(parts, 99000 + f))
    K = len(clusters) + len(snakes)
    expect = dict(K=[K] * 3, n_dyn=[n_dyn] * 3, dropped=[n_small] * 3, outside=[n_out] * 3, sizes={151, 159, 187, 199, 6, 8, 9, 12, 16},
                  hungarian=[None, (n_dyn, n_dyn), (n_dyn, n_dyn)], steps=[None, "<=2N", "<=2N"], in_map=False,
                  snakes=[(p, sn[4]) for p, sn in zip(fixed, snakes)], n_points=6144, min_cells=4500, min_K=300)
    return Scene("dense", frames, expect)


BUILDERS = {
    "k_edge_63": lambda: k_edge(63), "k_edge_64": lambda: k_edge(64), "k_edge_65": lambda: k_edge(65),
    "k_edge_128": lambda: k_edge(128), "k_edge_129": lambda: k_edge(129),
    "hungarian_edge": hungarian_edge, "all_gated_128": lambda: all_gated(128), "dense": dense, "rand_wrap": rand_wrap,
}


@functools.lru_cache(None)
def scene(name):
    return BUILDERS[name]()


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle's matching, restated with a step counter (oracle/dsp_oracle.c:hungarian, loop for loop)
def cost_matrix(dyn, last):
    """:1459-1472 in fp32: dyn / last = (n, 4) arrays cx, cy, cz, point_num"""
    dyn, last = np.asarray(dyn, F), np.asarray(last, F)
    e = (dyn[:, None, :3] - last[None, :, :3]).astype(F)
    d = np.sqrt(F(F(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])).astype(F)
    dn = np.abs(dyn[:, None, 3].astype(np.int64) - last[None, :, 3].astype(np.int64))
    gated = (dn > 100) | (d >= F(1.5))
    return np.where(gated, F(1.5) * F(5000.0), (d / F(1.5)).astype(F) * F(1000.0)).astype(F), ~gated


def hungarian_steps(cost):
    """(assign, steps): the oracle's algorithm on cost (nr x nc, fp32) and the number of passes through its do-while body"""
    cost = np.asarray(cost, F)
    nr, nc = cost.shape
    n = max(nr, nc)
    a = np.full((n + 1, n + 1), float(cost.max()) if cost.size else 0.0)
    a[1:nr + 1, 1:nc + 1] = cost
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    steps = 0
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, 1e300)
        used = np.zeros(n + 1, bool)
        while True:
            steps += 1
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = a[i0] - u[i0] - v
            upd = free & (cur < minv)
            minv[upd] = cur[upd]
            way[upd] = j0
            cand = np.where(free, minv, np.inf)
            j1 = int(np.argmin(cand))            # first minimum = the sequential loop's strict <
            delta = cand[j1]
            np.add.at(u, p[used], delta)
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    assign = np.full(nr, -1, np.int64)
    for j in range(1, n + 1):
        if 1 <= p[j] <= nr and j <= nc:
            assign[p[j] - 1] = j - 1
    return assign, steps


# ------------------------------------------------------------------------------------------------------------------------------------
_ORACLE_RUNS = {}
NEWBORN = 1


def oracle_run(orc, name, seed=1):
    """the oracle's frames of a scene, computed once per process and shared by the tests: per frame the birth cloud and the cursors.

    ONE newborn particle per birth source (NEWBORN; the handles under test are set up the same way): with the usual 20 the number of
    rand() draws of a point of an unmatched cluster is 20 - max(3, (int)(16 p_static)) of the mass in the point's voxel (:850-866),
    and the masses of two implementations agree to 1e-6 only -- a cluster that appears over particles of earlier frames would take
    the rand() cursors apart and, with them, the intensities of every later frame.  With one child the split is (int)(0 * p) = 0:
    every possibly-dynamic point inside the map draws three numbers, and both cursors are functions of the birth cloud alone."""
    from tests import common
    if name not in _ORACLE_RUNS:
        sc = scene(name)
        o = orc.Oracle(orc.make_config(**CFG))
        o.set_tables(*common.tables(seed))
        o.L.dspo_set_newborn_number(o.h, NEWBORN)
        o.L.dspo_use_velocity_estimator(o.h, 1)
        if sc.r_cursor is not None:
            o.L.dspo_set_cursors(o.h, 0, 0, sc.r_cursor)
        out = []
        for f, pts in enumerate(sc.frames):
            assert o.update(pts, sc.pos, sc.stamp(f), sc.quat) == 1
            out.append(dict(birth=o.get_birth_cloud().copy(), cursors=o.cursors()))
            o.get_occupancy_with_future(0.2)
        o.close()
        _ORACLE_RUNS[name] = out
    return _ORACLE_RUNS[name]
