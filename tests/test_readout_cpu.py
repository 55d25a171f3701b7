"""Pins tests/readout_ref.py to the CPU oracle, without a GPU: Oracle.get_occupancy_with_future(thr) (getOccupancyMapWithFutureStatus
:405-426) equals occupied_list(cfg, o.results[:, 0], thr) bit for bit -- the count, the order and the bits of every centre -- on
states whose masses vary: random particles with random weights injected and resampled, and three frames of the scaled wall cloud.
With thr = -1 the oracle lists all V centres, which pins the position arithmetic independently of any state."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import readout_ref as R

F = np.float32
RES = 0.15
SHAPES = [(3, 3, 3), (66, 12, 8), (18, 14, 6)]
IDS = ["3x3x3", "66x12x8", "18x14x6"]


def _injected(orc, shape, seed=5):
    """four particles per voxel on average, weights 0.002 .. 0.08, then occupancy_resample: masses around 0.16, all different"""
    cfg = orc.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12)
    o = orc.Oracle(cfg)
    px, py, pz, vx, vy, w = common.random_particles(seed, 4 * o.V, common.half_extent(cfg))
    o.inject(px, py, pz, vx, vy, np.zeros_like(px), w)
    o.occupancy_resample()
    return o


def _frames(orc, shape, dist):
    cfg = orc.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12)
    o = orc.Oracle(cfg)
    o.set_tables(*common.tables(7))
    pts = (common.wall_cloud(3, n_side=40) * F(dist / 3.0)).astype(F)
    s2 = float(np.sqrt(0.5))
    for f, quat in enumerate(((s2, 0.0, 0.0, s2), (0.0, 0.0, 0.0, 1.0), (1.0, 0.0, 0.0, 0.0))):
        assert o.update(pts, (0.0, 0.0, 0.0), f / 30.0, quat) == 1
    return o


def thresholds(mass):
    """the thresholds of a state: (name, thr); m0 = the median positive mass, a value that occurs in the grid"""
    pos = np.sort(mass[mass > 0])
    m0 = F(pos[len(pos) // 2])
    return m0, [("0.2", 0.2), ("m0", float(m0)), ("below m0", float(np.nextafter(m0, F(-np.inf)))), ("0", 0.0), ("-1", -1.0),
                ("+inf", float("inf")), ("nan", float("nan"))]


def _check(o, tiny, levels):
    cfg, V = o.cfg, o.V
    mass = o.results[:, 0].copy()
    assert len(np.unique(mass[mass > 0])) >= levels                                    # varied masses
    m0, thrs = thresholds(mass)
    counts = {}
    for name, thr in thrs:
        xo, _ = o.get_occupancy_with_future(thr)
        n, xyz = R.occupied_list(cfg, mass, thr)
        counts[name] = n
        assert xo.dtype == np.float32 and xo.shape == (n, 3), (name, xo.shape, n)
        assert xo.tobytes() == xyz.tobytes(), (name, np.flatnonzero((xo != xyz).any(1))[:5])
        assert np.array_equal(o.results[:, 0], mass)                                   # the readout leaves the masses alone
    n_m0 = int((mass == m0).sum())
    assert n_m0 >= 1 and counts["below m0"] == counts["m0"] + n_m0                     # strict >: a voxel of exactly thr is excluded
    assert counts["-1"] == V and counts["+inf"] == 0 and counts["nan"] == 0
    assert counts["0"] == int((mass > 0).sum())
    if not tiny:
        assert 0 < counts["0.2"] < counts["0"]
    # thr = -1: every centre, against the oracle's own per-index accessor
    x, y, z = C.c_float(), C.c_float(), C.c_float()
    all_xyz = R.occupied_list(cfg, mass, -1.0)[1]
    for i in (0, 1, cfg.nx - 1, cfg.nx, cfg.nx * cfg.ny - 1, cfg.nx * cfg.ny, V - 1):
        o.L.dspo_voxel_center(o.h, i, C.byref(x), C.byref(y), C.byref(z))
        assert np.array_equal(all_xyz[i], np.array([x.value, y.value, z.value], F)), i


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_equals_the_oracle_on_an_injected_state(orc, shape):
    o = _injected(orc, shape)
    _check(o, shape == (3, 3, 3), 5 if shape == (3, 3, 3) else 50)
    o.close()


@pytest.mark.parametrize("shape,dist", [((66, 12, 8), 4.0), ((18, 14, 6), 0.9)], ids=["66x12x8", "18x14x6"])
def test_restatement_equals_the_oracle_after_frames(orc, shape, dist):
    o = _frames(orc, shape, dist)
    _check(o, False, 10)      # (after three frames the masses are multiples of one newborn weight: many voxels AT a threshold m0)
    o.close()


def test_slab_base_shifts_the_index_not_the_order():
    """v_base: the list of a slab's mass column is the slice of the whole map's list that falls into the slab"""
    class Cfg:
        nx, ny, nz, voxel_resolution = 5, 4, 6, RES
    rng = np.random.default_rng(1)
    mass = rng.uniform(0.0, 0.4, 5 * 4 * 6).astype(F)
    n, xyz = R.occupied_list(Cfg, mass, 0.2)
    parts = []
    for z0, z1 in ((0, 1), (1, 4), (4, 6)):
        a, b = z0 * 20, z1 * 20
        k, p = R.occupied_list(Cfg, mass[a:b], 0.2, v_base=a)
        assert k == int((mass[a:b] > F(0.2)).sum())
        parts.append(p)
    assert 0 < n < mass.size and np.concatenate(parts).tobytes() == xyz.tobytes()
