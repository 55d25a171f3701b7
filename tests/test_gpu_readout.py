"""GPU tests of the occupied-voxel readout (dspmap_get_occupancy, dspmap_get_occupancy_with_future: k_occ_count, k_occ_scan, k_occ_emit):
zero differing bits -- the count, the order and every coordinate -- against the numpy restatement (tests/readout_ref.py, pinned to the
CPU oracle by tests/test_readout_cpu.py) over the same handle's results()[:, 0], read in the same quiescent state.

Shapes, each the smallest at which its edge exists: 3 x 3 x 3 (one partial wave), 66 x 12 x 8 (6 336 voxels = 24.75 blocks: wave edges
inside blocks, a ragged last block), 18 x 14 x 6 under both storage orders (cubes padded on all three axes), 130 x 64 x 32 (266 240 voxels
= 1 040 blocks: k_occ_scan's loop makes a second trip with 16 of its 1 024 lanes in use) and 2- and 4-slab groups of 40 x 40 x 24 with
slabs of unequal height (v_base != 0).  Thresholds per state: 0.2, the median positive mass m0 (strict >: voxels of exactly m0 are
excluded), the float below m0 (now included), 0, -1 (all V voxels), +inf and NaN (none).

Before it compares, every test asserts on the RESTATEMENT's side that the grid is not degenerate."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import common
from tests import readout_ref as R
from tests.test_gpu_frontier import QUATS, _cloud
from tests.test_gpu_query import _slab_stream

pytestmark = pytest.mark.gpu
F = np.float32
RES = 0.15
TINY, WIDE, PADDED, LARGE = (3, 3, 3), (66, 12, 8), (18, 14, 6), (130, 64, 32)
SENTINEL = F(-12345.0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _particles(cfg, slots, seed, per_voxel=2.0):
    """random particles with random weights, (voxel, slot, rec8) for import_state: per_voxel on average (so some voxels stay empty and
    some pass five particles and are resampled), half of them moving, weights 0.002 .. 0.2 (a voxel's mass straddles 0.2)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = cfg.nx, cfg.ny, cfg.nz
    V = nx * ny * nz
    n = int(per_voxel * V)
    vox = np.sort(rng.integers(0, V, n))
    slot = np.arange(n) - np.searchsorted(vox, vox, side="left")          # rank within the voxel
    keep = slot < slots
    vox, slot = vox[keep], slot[keep]
    n = len(vox)
    hx, hy, hz = common.half_extent(cfg)
    iz, iy, ix = vox // (nx * ny), (vox // nx) % ny, vox % nx
    rec = np.zeros((n, 8), F)
    rec[:, 0] = 1.0
    moving = rng.random(n) > 0.5
    rec[:, 1] = rng.uniform(-0.8, 0.8, n) * moving
    rec[:, 2] = rng.uniform(-0.8, 0.8, n) * moving
    for a, (i, h) in enumerate(((ix, hx), (iy, hy), (iz, hz))):
        rec[:, 4 + a] = -h + (i + rng.uniform(0.05, 0.95, n)) * RES       # inside the voxel, away from its faces
    rec[:, 7] = rng.uniform(0.002, 0.2, n)
    return vox.astype(np.int32), slot.astype(np.int32), rec


def _injected(dsp, shape, tiling=None, seed=5):
    """a handle with the random particles imported and resampled once (masses and future status of the whole map)"""
    cfg = dsp.make_config(nx=shape[0], ny=shape[1], nz=shape[2], res=RES, ppv=12, seed=7)
    m = dsp.DSPMap(cfg)
    if tiling is not None:
        m.set_param(dsp.capi.P_TILING, tiling)
    vox, slot, rec = _particles(cfg, m.slots, seed)
    m.clear_state()
    m.import_state(vox, rec, slot)
    m.clearOccupancyMapPrediction()
    m.occupancy_resample()
    if tiling is not None:
        assert int(m.get_param(dsp.capi.P_TILING)) == tiling
    return m


def _thresholds(mass):
    """(m0, [(name, thr, interior)]): m0 = the median positive mass, a value that occurs in the grid"""
    pos = np.sort(mass[mass > 0])
    assert pos.size >= 5
    m0 = F(pos[len(pos) // 2])
    return m0, [("0.2", 0.2, True), ("m0", float(m0), True), ("below m0", float(np.nextafter(m0, F(-np.inf))), True), ("0", 0.0, False),
                ("-1", -1.0, False), ("+inf", float("inf"), False), ("nan", float("nan"), False)]


def _non_degenerate(mass, share=True):
    """on the restatement's input: varied masses; at each interior threshold both classes hold at least 5 % of the voxels that carry mass;
    a voxel of exactly m0 is excluded at m0 and included just below"""
    m0, thrs = _thresholds(mass)
    carrying = int((mass > 0).sum())
    assert len(np.unique(mass[mass > 0])) >= 5
    for name, thr, interior in thrs:
        if interior and share:
            above = int((mass > F(thr)).sum())
            assert above >= 0.05 * carrying and carrying - above >= 0.05 * carrying, (name, above, carrying)
    at = np.flatnonzero(mass == m0)
    assert at.size >= 1
    assert not (mass[at] > F(thrs[1][1])).any() and (mass[at] > F(thrs[2][1])).all()
    return m0, thrs


def _raw(m, thr, cap, with_future=False, null=False):
    """the raw entry point into a sentinel-filled buffer of V_local + 1 triples: (rc, n, buffer[, future])"""
    buf = np.full((m.V_local + 1, 3), SENTINEL, F)
    n = C.c_int(-1)
    ptr = None if null else _p(buf)
    if with_future:
        fut = np.full((m.V_local, m.T), SENTINEL, F)
        rc = m.L.dspmap_get_occupancy_with_future(m.h, thr, ptr, cap, C.byref(n), _p(fut))
        return rc, n.value, buf, fut
    rc = m.L.dspmap_get_occupancy(m.h, thr, ptr, cap, C.byref(n))
    return rc, n.value, buf


def _check_lists(m, mass, thrs, v_base=0, tag=None):
    """every threshold through the wrapper (cap = V_local): count, order and bits; returns {name: (n, xyz)} of the restatement"""
    want = {}
    for name, thr, _ in thrs:
        n, xyz = R.occupied_list(m.cfg, mass, thr, v_base=v_base)
        ng, xg = m.getOccupancyMap(thr)
        assert ng == n == len(xg), (tag, name, ng, n, len(xg))
        bad = np.flatnonzero((xg.view(np.uint32) != xyz.view(np.uint32)).any(1))
        assert bad.size == 0, (tag, name, bad.size, bad[:5], xg[bad[:5]], xyz[bad[:5]])
        want[name] = (n, xyz)
    assert want["-1"][0] == m.V_local and want["+inf"][0] == 0 and want["nan"][0] == 0
    return want


def _check_raw(m, thrs, want, tag=None):
    """cap = n // 2 (a prefix, the rest of the buffer untouched, *n_out = n), cap = 0 with xyz = NULL, a full-size cap; the with_future
    entry point returns the same list"""
    for name, thr, _ in thrs:
        n, xyz = want[name]
        cap = n // 2
        rc, ng, buf = _raw(m, thr, cap)
        assert rc == 1 and ng == n, (tag, name, rc, ng, n)
        assert buf[:cap].tobytes() == xyz[:cap].tobytes() and (buf[cap:] == SENTINEL).all(), (tag, name, "cap = n // 2")
        rc, ng, buf = _raw(m, thr, 0, null=True)
        assert rc == 1 and ng == n and (buf == SENTINEL).all(), (tag, name, "cap = 0, NULL")
        rc, ng, buf = _raw(m, thr, m.V_local)
        assert rc == 1 and ng == n and buf[:n].tobytes() == xyz.tobytes() and (buf[n:] == SENTINEL).all(), (tag, name, "cap = V")
        rc, ng, buf, _fut = _raw(m, thr, m.V_local, with_future=True)
        assert rc == 1 and ng == n and buf[:n].tobytes() == xyz.tobytes() and (buf[n:] == SENTINEL).all(), (tag, name, "with future")


def _check_future_and_repeats(m, twin, thr):
    """the future array of the readout equals getFutureStatus() of the identical twin read immediately before; two readouts in a row give
    identical bytes; a readout leaves export_state() and results() unchanged"""
    res, state = m.results(), m.export_state()
    assert np.array_equal(res, twin.results())
    for a, b in zip(state, twin.export_state()):
        assert np.array_equal(a, b)
    fa = twin.getFutureStatus()
    assert (fa != 0).any()
    n1, x1, f1 = m.getOccupancyMapWithFutureStatus(thr)
    assert f1.tobytes() == fa.tobytes()
    n2, x2 = m.getOccupancyMap(thr)
    n3, x3 = m.getOccupancyMap(thr)
    assert n1 == n2 == n3 and x1.tobytes() == x2.tobytes() == x3.tobytes()
    assert np.array_equal(m.results(), res)
    for a, b in zip(state, m.export_state()):
        assert np.array_equal(a, b)
    return f1


@pytest.mark.parametrize("shape", [TINY, WIDE], ids=["3x3x3", "66x12x8"])
def test_readout_equals_the_restatement(dsp, shape):
    m, twin = _injected(dsp, shape), _injected(dsp, shape)
    mass = m.results()[:, 0].copy()
    m0, thrs = _non_degenerate(mass, share=shape != TINY)
    print(shape, "voxels with mass", int((mass > 0).sum()), "above 0.2", int((mass > F(0.2)).sum()), "m0", float(m0))
    _check_future_and_repeats(m, twin, float(m0))         # (first: a readout arms the clear of the future status)
    want = _check_lists(m, mass, thrs, tag=shape)
    _check_raw(m, thrs, want, tag=shape)
    m.close(), twin.close()


def test_readout_under_both_storage_orders(dsp):
    """18 x 14 x 6: 4 x 4 x 4 cubes padded on all three axes; the lists of the two storage orders are identical bytes"""
    cubes, runs = _injected(dsp, PADDED, tiling=1), _injected(dsp, PADDED, tiling=0)
    res_c, res_r = cubes.results(), runs.results()
    assert np.array_equal(res_c, res_r)
    mass = res_c[:, 0].copy()
    m0, thrs = _non_degenerate(mass)
    twin = _injected(dsp, PADDED, tiling=1)
    fut = _check_future_and_repeats(cubes, twin, float(m0))                                # (first: a readout arms the clear)
    assert runs.getOccupancyMapWithFutureStatus(float(m0))[2].tobytes() == fut.tobytes()   # the future array is in voxel order too
    want = _check_lists(cubes, mass, thrs, tag="cubes")
    _check_lists(runs, mass, thrs, tag="runs")
    _check_raw(cubes, thrs, want, tag="cubes")
    for name, thr, _ in thrs:
        (nc, xc), (nr, xr) = cubes.getOccupancyMap(thr), runs.getOccupancyMap(thr)
        assert nc == nr and xc.tobytes() == xr.tobytes(), name
    assert int(cubes.get_param(dsp.capi.P_TILING)) == 1 and int(runs.get_param(dsp.capi.P_TILING)) == 0
    cubes.close(), runs.close(), twin.close()


def test_readout_past_one_trip_of_the_block_scan(dsp):
    """130 x 64 x 32 = 266 240 voxels = 1 040 blocks: k_occ_scan's loop runs twice, the second trip over the last 16 blocks.  Seeded with two
    moving particles per voxel, then two frames of the scaled wall cloud."""
    t0 = time.perf_counter()
    cfg = dsp.make_config(nx=LARGE[0], ny=LARGE[1], nz=LARGE[2], res=RES, ppv=9, seed=7)
    m = dsp.DSPMap(cfg)
    V = m.V
    assert V == 266240 and (V + 255) // 256 == 1040
    m.seed_uniform(2, 0.1, 17, vmax=0.8)
    pts = _cloud(4.0)
    for f, quat in enumerate((QUATS["identity"], QUATS["yaw90"])):
        assert m.update(pts, (0.0, 0.0, 0.0), f / 30.0, quat) == 1
    mass = m.results()[:, 0].copy()
    m0, thrs = _non_degenerate(mass)
    for name, thr, interior in thrs:
        if interior:                                      # occupied voxels in both trips' block ranges; the last 16 blocks ARE the second trip
            blocks = np.flatnonzero(mass > F(thr)) // 256
            first, second = int((blocks < 1024).sum()), int((blocks >= 1024).sum())
            assert first > 0 and second > 0 and len(np.unique(blocks[blocks >= 1024])) >= 8, (name, first, second)
    print("voxels with mass", int((mass > 0).sum()), "above 0.2", int((mass > F(0.2)).sum()), "m0", float(m0), "levels", len(np.unique(mass)))
    want = _check_lists(m, mass, thrs, tag=LARGE)
    _check_raw(m, thrs[:3], want, tag=LARGE)
    n1, x1 = m.getOccupancyMap(0.2)
    n2, x2 = m.getOccupancyMap(0.2)
    assert n1 == n2 and x1.tobytes() == x2.tobytes() and np.array_equal(m.results()[:, 0], mass)
    m.close()
    print("266 240-voxel case: %.2f s" % (time.perf_counter() - t0))


RANGES = {2: [(0, 10), (10, 24)], 4: [(0, 5), (5, 12), (12, 17), (17, 24)]}


@pytest.mark.parametrize("world", [2, 4])
def test_readout_of_slabs(dsp, world):
    """slabs of unequal height through the group driver: each slab's list is the restatement's with v_base = the slab's first voxel, and the
    lists in rank order are the list of the concatenated results"""
    sharded = __import__("dsp-map_amd.sharded", fromlist=["CppGroup"])
    kw = dict(nx=40, ny=40, nz=24, res=RES, ppv=12)
    tables = common.tables(3)
    grp = sharded.CppGroup(dsp, kw, world, ranges=RANGES[world])
    for m in grp.maps:
        m.set_tables(*tables)
    for f, (pts, pos, t, q) in enumerate(_slab_stream(6)):
        d = torch.from_numpy(pts).cuda()
        assert grp.update(d, pos, t, q) == 1
        grp.sync()
        if f < 5:
            for m in grp.maps:
                m.clearOccupancyMapPrediction()
    cfg = dsp.make_config(**kw)                           # the whole map's dimensions
    masses = [m.results()[:, 0].copy() for m in grp.maps]
    bases = [m.L.dspmap_local_voxel_base(m.h) for m in grp.maps]
    assert bases == [z0 * 40 * 40 for z0, _ in RANGES[world]] and [len(x) for x in masses] == [(z1 - z0) * 1600 for z0, z1 in RANGES[world]]
    whole = np.concatenate(masses)
    m0, thrs = _non_degenerate(whole)
    assert sum(int((x > F(0.2)).any()) for x in masses) >= 2                             # more than one slab has something to list
    per_slab = []
    for r, m in enumerate(grp.maps):
        assert m.V_local == len(masses[r]) and m.V == 38400
        want = _check_lists(m, masses[r], thrs, v_base=bases[r], tag=("slab", r))
        _check_raw(m, thrs[:3], want, tag=("slab", r))
        per_slab.append(want)
        assert np.array_equal(m.results()[:, 0], masses[r])
    for name, thr, _ in thrs:
        n, xyz = R.occupied_list(cfg, whole, thr)
        assert n == sum(w[name][0] for w in per_slab)
        assert np.concatenate([m.getOccupancyMap(thr)[1] for m in grp.maps]).tobytes() == xyz.tobytes(), name
    grp.close()
