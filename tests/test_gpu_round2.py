"""GPU parity tests for the corner cases closed in round 2 (run with `-m gpu` on an MI355X)."""
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tests.test_gpu_parity import RTOL, gpu_state, make_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slots_equal(o, m, cols=(0, 1, 2, 3, 4, 5, 6)):
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    assert len(vo) == len(vg)
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    assert np.array_equal(vo[ko], vg[kg]) and np.array_equal(so[ko], sg[kg])
    for c in cols:
        assert np.array_equal(ro[ko][:, c], rg[kg][:, c]), c
    return ro[ko], rg[kg]


def test_prefill_then_first_frame_births_skip_prefilled_slots(dsp, orc):
    """DSPMap(init_particle_num > 0) followed by the first update(): addAParticle (:1184-1185) skips every slot whose flag
    is >= 0.1 -- including the pre-filled particles, which still carry the newborn flag 15 -- so the first frame's
    newborns take the free slots BEHIND them.  Birth stage from the pre-filled state: same particles in the same slots."""
    cfgkw = dict(nx=30, ny=30, nz=16, ppv=10)
    o, m = make_pair(dsp, orc, **cfgkw)
    n = 20000
    o.L.dspo_add_random_particles(o.h, n, 0.01)
    m._chk(m.L.dspmap_add_random_particles(m.h, n, 0.01))
    pts = common.wall_cloud(2, n_side=30, dist=1.6, half_w=1.2, half_h=0.7)
    for x in (o, m):
        x.bin_points(pts)
        x.predict(0, 0, 0, 0)         # flag-15 particles are not predicted (:649)
        x.map_update()
    o.L.dspo_use_velocity_estimator(o.h, 2)
    o.L.dspo_static_birth_cloud(o.h)
    o.add_newborn(); m.add_newborn()
    ro, rg = _slots_equal(o, m)
    assert (ro[:, 0] > 10).sum() > n                       # pre-filled + this frame's newborns, all flagged 15
    assert np.allclose(ro[:, 7], rg[:, 7], rtol=RTOL)
    # a second birth stage without a resampling in between: the first stage's newborns are skipped as well
    o.add_newborn(); m.add_newborn()
    ro, rg = _slots_equal(o, m)
    # ... and the whole first frames of both, through update()
    o2, m2 = make_pair(dsp, orc, **cfgkw)
    o2.L.dspo_add_random_particles(o2.h, n, 0.01)
    m2._chk(m2.L.dspmap_add_random_particles(m2.h, n, 0.01))
    o2.L.dspo_use_velocity_estimator(o2.h, 2)
    assert o2.update(pts, (0, 0, 0), 0.0, (1, 0, 0, 0)) == 1 and m2.update(pts, (0, 0, 0), 0.0, (1, 0, 0, 0)) == 1
    # (which of a voxel's EQUAL-weight newborns survive the resampling is a threshold tie, see DESIGN "numerics": compare
    # the per-voxel population and mass, and the pre-filled particles, none of which is resampled away or overwritten)
    vo, so, r2o = o2.export_sparse()
    vg, sg, r2g = gpu_state(m2)
    assert np.array_equal(np.bincount(vo, minlength=o2.V), np.bincount(vg, minlength=o2.V))
    assert np.allclose(m2.results()[:, 0], o2.results[:, 0], rtol=RTOL, atol=1e-6)
    pre_o, pre_g = r2o[r2o[:, 3] != 0], r2g[r2g[:, 3] != 0]          # pre-filled particles still carry their vz
    assert len(pre_o) == len(pre_g) > 0.9 * n
    a_v, a_r = common.sorted_records(vo[r2o[:, 3] != 0], pre_o, cols=(4, 5, 6, 1, 2, 3))
    b_v, b_r = common.sorted_records(vg[r2g[:, 3] != 0], pre_g, cols=(4, 5, 6, 1, 2, 3))
    assert np.array_equal(a_v, b_v) and np.array_equal(a_r[:, 1:7], b_r[:, 1:7])
    for x in (o, m, o2, m2):
        x.close()


def test_static_model_births_from_sources_outside_the_map(dsp, orc):
    """dsp_static.h:797-825 has no voxel lookup for the source point: a point of the view that lies outside the map box
    still draws its 3 x n position values and places the children that land inside.  The map is made shallower than the
    wall's distance so that sources sit just outside the front face."""
    cfg = dict(nx=20, ny=30, nz=16, res=0.2, ppv=10, half_fov_v=27, pred_times=(0.05,), safe_factor=5, static_model=1)
    o, m = make_pair(dsp, orc, **cfg)          # half_x = 2.0
    pts = common.wall_cloud(4, n_side=40, dist=2.03, half_w=1.6, half_h=0.8, wav=0.04)   # x in ~[1.97, 2.09]: both sides of the face
    assert (pts[:, 0] > 2.0).sum() > 100 and (pts[:, 0] < 2.0).sum() > 100
    for x in (o, m):
        x.bin_points(pts)
        x.predict(0, 0, 0, 0)
        x.map_update()
    o.L.dspo_static_birth_cloud(o.h)
    o.add_newborn(); m.add_newborn()
    assert o.cursors() == m.cursors()          # every source consumed its draws, inside the map or not
    ro, rg = _slots_equal(o, m)
    assert len(ro) > 3000
    o.close(); m.close()


@pytest.mark.parametrize("static_model", [0, 1])
def test_empty_view_reuses_previous_birth_cloud(dsp, orc, static_model):
    """velocityEstimationThread returns before clearing its output when the view is empty (:1379-1381,
    dsp_static.h:1288-1290): the birth stage then re-uses the last non-empty view's cloud, shifted by the new sensor
    position"""
    cfg = dict(nx=30, ny=30, nz=16, res=0.2, ppv=20)
    if static_model:
        cfg.update(half_fov_v=27, pred_times=(0.05,), safe_factor=5, static_model=1)
    o, m = make_pair(dsp, orc, **cfg)
    o.L.dspo_use_velocity_estimator(o.h, 2)
    # two children per source keep every voxel below MAX_PARTICLE_NUM_VOXEL: no equal-weight resampling ties (DESIGN
    # "numerics"), so the two sides stay comparable particle by particle over the frames
    o.L.dspo_set_newborn_number(o.h, 2); m.setNewBornParticleNumberofEachPoint(2)
    wall = common.wall_cloud(6, n_side=30, dist=1.8, half_w=1.2, half_h=0.7)
    behind = wall.copy(); behind[:, 0] *= -1.0                      # every point outside the field of view
    few_behind = behind[:7]
    clouds = [wall, behind, few_behind, np.zeros((0, 3), np.float32), wall[:500]]
    for f, pts in enumerate(clouds):
        pos = (0.02 * f, 0.01 * f, 0.0)
        assert o.update(pts, pos, f / 30.0, (1, 0, 0, 0)) == 1
        assert m.update(pts, pos, f / 30.0, (1, 0, 0, 0)) == 1
        assert o.cursors()[0] == m.cursors()[0], f                     # the stale cloud drew its position values again
        c = m.counters()
        if f in (1, 2, 3):
            assert c["n_valid"] == 0 and c["n_born"] > 300, (f, c)     # births without a single observation
        bo, bg = o.get_birth_cloud(), m.get_birth_cloud()
        assert len(bo) == len(bg) and np.array_equal(bo["x"], bg["x"]) and np.array_equal(bo["z"], bg["z"]), f
        occ_o, occ_g = o.results[:, 0].astype(np.float64), m.results()[:, 0].astype(np.float64)
        assert abs(occ_g.sum() - occ_o.sum()) < 2e-3 * occ_o.sum(), f
        o.get_occupancy_with_future(0.2); m.getOccupancyMapWithFutureStatus(0.2)
    # the same through the captured device-resident frame
    import torch
    m3 = dsp.DSPMap(dsp.make_config(**cfg)); m3.set_tables(*common.tables(1)); m3.setNewBornParticleNumberofEachPoint(2)
    for f, pts in enumerate(clouds):
        t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
        assert m3.update_device(t.data_ptr(), len(pts), (0.02 * f, 0.01 * f, 0.0), f / 30.0, (1, 0, 0, 0)) == 1
        m3.getOccupancyMapWithFutureStatus(0.2)
    for a, b in zip(m.export_state(), m3.export_state()):
        assert np.array_equal(a, b)
    o.close(); m.close(); m3.close()


def test_resample_copies_into_the_second_occupancy_word(dsp, orc):
    """more than 64 live particles in a voxel of a 72-slot map: copies made while the first occupancy word is walked land
    in the second word and must not be revisited there (they carry flag 0.6, :1009)"""
    cfgkw = dict(nx=10, ny=10, nz=6, res=0.10, ppv=36)
    o, m = make_pair(dsp, orc, **cfgkw)
    assert m.slots == 72
    rng = np.random.default_rng(3)
    px, py, pz, w = [], [], [], []
    for k, (cx, cy, cz) in enumerate([(0.05, 0.05, 0.05), (0.15, -0.25, 0.15), (-0.35, 0.25, -0.05)]):
        n = (66, 70, 40)[k]                                   # 66 / 70 occupy both words; the resampler keeps 36
        px += list(cx + rng.uniform(-0.04, 0.04, n)); py += list(cy + rng.uniform(-0.04, 0.04, n)); pz += list(cz + rng.uniform(-0.04, 0.04, n))
        ww = rng.uniform(0.002, 0.01, n)
        ww[:3] = (0.9, 0.6, 0.4)                              # heavy early particles: several copies each
        w += list(ww)
    px, py, pz, w = (np.asarray(a, np.float32) for a in (px, py, pz, w))
    z = np.zeros(len(px), np.float32)
    common.inject_both(o, m, px, py, pz, z, z, w)
    cnt = np.bincount(o.export_sparse()[0], minlength=o.V)
    assert cnt.max() == 70
    # free a few low slots so that copies are spread over both words
    o.occupancy_resample(); m.occupancy_resample()
    assert np.array_equal(m.results()[:, 0], o.results[:, 0])
    ro, rg = _slots_equal(o, m, cols=(4, 5, 6))
    assert np.allclose(ro[:, 7], rg[:, 7], rtol=1e-6)
    # a second pass over the resampled state (survivors + copies, now all flag 1)
    o.occupancy_resample(); m.occupancy_resample()
    ro, rg = _slots_equal(o, m, cols=(4, 5, 6))
    o.close(); m.close()


def _fill_view(o, m, n, seed, vmax=0.0):
    half = common.half_extent(o.cfg)
    rng = np.random.default_rng(seed)
    # inside the field of view (x forward, +-42 / +-24 degrees), spread over the map's depth
    r = rng.uniform(0.3, half[0] * 0.95, n)
    az = np.radians(rng.uniform(-40, 40, n)); el = np.radians(rng.uniform(-22, 22, n))
    px = (r * np.cos(az)).astype(np.float32); py = (r * np.sin(az)).astype(np.float32)
    pz = (r * np.cos(az) * np.tan(el)).astype(np.float32)
    keep = (np.abs(py) < half[1] * 0.98) & (np.abs(pz) < half[2] * 0.98) & (np.abs(px) < half[0] * 0.98)
    px, py, pz = px[keep], py[keep], pz[keep]
    vx = (rng.uniform(-vmax, vmax, len(px))).astype(np.float32)
    vy = (rng.uniform(-vmax, vmax, len(px))).astype(np.float32)
    w = rng.uniform(0.01, 0.05, len(px)).astype(np.float32)
    return common.inject_both(o, m, px, py, pz, vx, vy, w)


def test_pyramid_list_overflow_in_sweep_order(dsp, orc):
    """pyramid-list overflow (-2, :1245-1259): a pyramid registers at most SAFE_PARTICLE_NUM_PYRAMID particles, in the
    order of the reference's voxel / slot sweep; the ones that come later are removed.  Every list entry carries its sweep
    key and k_pyr_prepare keeps the SAFE_PARTICLE_NUM_PYRAMID smallest keys of a full list: the same particles survive as in
    the oracle, in the same slots -- also when particles change voxel: a slot handed back by a turned-away particle is
    re-used by the arrivals behind it in the sweep (k_place_fix)."""
    cfgkw = dict(nx=40, ny=40, nz=10, res=0.15, ppv=9)
    o, m = make_pair(dsp, orc, **cfgkw)
    assert m.capp == o.capp == 66
    n_in = _fill_view(o, m, 90000, 8)
    empty = np.zeros((0, 3), np.float32)
    o.bin_points(empty); m.bin_points(empty)
    o.predict(0.0, 0.0, 0.0, 0.0); m.predict(0.0, 0.0, 0.0, 0.0)          # nobody moves: candidates = the particles in view
    len_o = (o.pyramid_lists[:, :, 0] != 0).sum(1)
    assert np.array_equal(len_o, m.pyramid_counts()) and (len_o == o.capp).sum() > 20   # many full lists
    c = m.counters()
    ro, rg = _slots_equal(o, m, cols=(1, 2, 4, 5, 6, 7))                   # the same particles in the same slots
    assert len(ro) == n_in - c["n_pyramid_full"] and c["n_pyramid_full"] > 500
    assert c["n_fov"] == int(len_o.sum())
    # a second frame on the survivors (lists full again), then the weight update on both
    o.predict(0.0, 0.0, 0.0, 0.0); m.predict(0.0, 0.0, 0.0, 0.0)
    _slots_equal(o, m, cols=(1, 2, 4, 5, 6, 7))
    o.close(); m.close()
    # with motion: movers and stayers compete for the list in sweep order
    o, m = make_pair(dsp, orc, **cfgkw)
    n_in = _fill_view(o, m, 90000, 9, vmax=1.5)
    o.bin_points(empty); m.bin_points(empty)
    o.predict(-0.03, 0.02, 0.0, 0.1); m.predict(-0.03, 0.02, 0.0, 0.1)
    len_o = (o.pyramid_lists[:, :, 0] != 0).sum(1)
    len_g = m.pyramid_counts()
    assert (len_o == o.capp).sum() >= 5, (len_o == o.capp).sum()
    c = m.counters()
    assert c["n_moved"] > 1000 and c["n_pyramid_full"] > 50 and c["n_reslotted"] > 5, c
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    same = len(vo) == len(vg) and np.array_equal(vo[ko], vg[kg]) and np.array_equal(so[ko], sg[kg]) and \
        np.array_equal(ro[ko][:, 1:8], rg[kg][:, 1:8])
    if c["n_overflow_inexact"] == 0:
        # k_place_fix hands the slots of turned-away particles to the arrivals behind them: lists and SLOTS as in the oracle
        assert np.array_equal(len_o, len_g) and same
    else:
        # the one coincidence the pass does not treat (an arrival that found its voxel full before the lists were cut and
        # would fit afterwards): counted, and bounded here
        assert (len_o != len_g).sum() <= 0.02 * o.NP and np.abs(len_o - len_g).max() <= 2, np.nonzero(len_o != len_g)
        key_o = set(map(tuple, np.column_stack([vo, ro[:, 4:7].view(np.int32)]).tolist()))
        key_g = set(map(tuple, np.column_stack([vg, rg[:, 4:7].view(np.int32)]).tolist()))
        assert len(key_o ^ key_g) <= 0.002 * len(key_o), (len(key_o), len(key_g), len(key_o ^ key_g), c["n_overflow_inexact"])
    o.close(); m.close()


def test_checkpoint_into_handle_with_other_tables(dsp, tmp_path):
    """a checkpoint restores the filter parameters but not the saving handle's table lengths: loading into a handle
    whose injected tables are shorter keeps every cursor inside them"""
    cfgkw = dict(nx=30, ny=30, nz=16, ppv=10)
    a = dsp.DSPMap(dsp.make_config(**cfgkw)); a.set_tables(*common.tables(1, n=200003, nrand=50021))
    pts = common.wall_cloud(2, n_side=30, dist=1.6, half_w=1.2, half_h=0.7)
    for f in range(3):
        assert a.update(pts, (0.01 * f, 0, 0), f / 30.0, (1, 0, 0, 0)) == 1
    path = str(tmp_path / "a.ck")
    a.save_checkpoint(path)
    assert a.cursors()[0] > 5003
    b = dsp.DSPMap(dsp.make_config(**cfgkw)); b.set_tables(*common.tables(2, n=5003, nrand=1009))
    b.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, 7.0)
    b.load_checkpoint(path)
    pc, vc, rc = b.cursors()
    assert 0 <= pc < 5003 and 0 <= vc < 5003 and 0 <= rc < 1009
    assert b.L.dspmap_get_param(b.h, dsp.capi.P_PAIR_CULL_SIGMAS) == 7.0
    for f in range(3, 6):
        assert b.update(pts, (0.01 * f, 0, 0), f / 30.0, (1, 0, 0, 0)) == 1
    assert b.counters()["n_live_out"] > 1000
    # a header with an absurd particle count is rejected, not thrown across the C ABI
    raw = bytearray(open(path, "rb").read())
    hdr_n = raw.find(np.int32(len(a.export_state()[0])).tobytes(), 0, 512)
    assert hdr_n > 0
    raw[hdr_n:hdr_n + 4] = np.int32(-5).tobytes()
    bad = str(tmp_path / "bad.ck")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(dsp.capi.DSPMapError):
        b.load_checkpoint(bad)
    a.close(); b.close()


def _cluster_scene(t, frame):
    """sensor-frame cloud: ground + six groups of non-ground points (sensor 1.0 m above the ground, identity attitude)"""
    def box(x0, y0, z0, nx, ny, nz, step=0.1):
        xs, ys, zs = np.meshgrid(x0 + step * np.arange(nx), y0 + step * np.arange(ny), z0 + step * np.arange(nz), indexing="ij")
        return np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)
    parts = []
    gx, gy = np.meshgrid(np.arange(2.3, 3.4, 0.1), np.arange(-1.6, 1.6, 0.1))
    parts.append(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -0.98)], 1))        # ground: z_world = 0.02 <= 0.1
    parts.append(box(2.0, -1.5 + 1.0 * t, -0.7, 1, 5, 12))                               # A: 60 points, 1 m/s along +y
    parts.append(box(3.9, 0.9 - 6.0 * t, -0.8, 1, 4, 20))                                # B: 80 points, 6 m/s: > 5 m/s -> zeroed
    parts.append(box(2.6, -0.2, -0.5, 1, 5, 6) if frame == 0 else box(2.6, -0.2, -0.5, 1, 10, 16))   # C: 30 -> 160 points: gated
    parts.append(box(4.2, -1.5, -0.8, 1, 30, 9))                                         # D: 270 points (> 200): static
    parts.append(box(2.2, 0.9, 0.55, 1, 4, 5))                                           # E: centre z_world 1.75 > 1.5: static
    parts.append(box(1.6, 1.2, -0.3, 1, 1, 3))                                           # F: 3 points: below the minimum size, dropped
    parts.append(box(3.6, 0.2 + 0.5 * t, -0.6, 1, 3, 8))                                 # G: 24 points, 0.5 m/s
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("mode", [1, 2])
def test_velocity_estimator_multi_cluster_against_oracle(dsp, orc, mode):
    """a17 on a scene with seven groups of points: four possibly-dynamic clusters (one faster than the 5 m/s limit,
    :1490-1493; one whose point count changes by more than 100 between frames, :1463), two static ones (> 200 points;
    centre higher than 1.5 m, :1436), one below the minimum cluster size (:1412): the birth cloud -- points, ORDER
    (clusters by size, indices ascending inside a cluster, then the static points), tags and velocities -- equals the
    oracle's restatement of velocityEstimationThread (:1377-1544).  mode 1: the host stage (velocity_estimator.cpp);
    mode 2: the device estimator (dspmap_velest.hip: connected components by union-find, one-wavefront Hungarian),
    which also draws the clusters' display intensities from the shared rand() table like the oracle"""
    cfgkw = dict(nx=66, ny=66, nz=40, ppv=9)
    o, m = make_pair(dsp, orc, **cfgkw)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, mode)
    o.L.dspo_use_velocity_estimator(o.h, 1)
    pos = (0.0, 0.0, 1.0)
    for f in range(3):
        t = f * 0.1
        pts = _cluster_scene(t, f)
        assert m.update(pts, pos, t, (1, 0, 0, 0)) == 1
        assert o.update(pts, pos, t, (1, 0, 0, 0)) == 1
        g, w = m.get_birth_cloud(), o.get_birth_cloud()
        assert len(g) == len(w) == len(pts) - 3, f                   # everything but the 3-point group
        for k in ("x", "y", "z"):
            assert np.array_equal(g[k], w[k]), (f, k)                # same points in the same ORDER
        dyn_g, dyn_w = g["intensity"] > 0.01, w["intensity"] > 0.01
        assert np.array_equal(dyn_g, dyn_w)
        n_c = 30 if f == 0 else 160
        assert dyn_g.sum() == 60 + 80 + n_c + 24, f                  # A, B, C, G are possibly dynamic; D and E are not
        for k in ("nx", "ny", "nz"):
            assert np.array_equal(g[k], w[k]), (f, k)
        if mode == 2:
            assert np.array_equal(g["intensity"], w["intensity"]), f
            # position and rand() streams stay in step (the velocity stream depends on the static/dynamic split of the
            # existing mass, :850-866, i.e. on weights that agree to 1e-6 only)
            assert o.cursors()[0] == m.cursors()[0] and o.cursors()[2] == m.cursors()[2], f
        # inside a cluster every point carries the same tag
        first = np.nonzero(dyn_g)[0]
        if f == 0:
            assert (g["nx"][dyn_g] < -100).all()                     # nothing to match against: sentinel -10000 (:104-106)
        else:
            vy = g["ny"][dyn_g]
            a = np.isclose(vy, 1.0, atol=0.02).sum(); gsel = np.isclose(vy, 0.5, atol=0.02).sum()
            assert a == 60 and gsel == 24, (f, a, gsel)              # A and G matched
            b_pts = (np.abs(g["x"] - 3.9) < 1e-3) & dyn_g
            assert b_pts.sum() == 80 and (g["nx"][b_pts] == 0).all() and (g["ny"][b_pts] == 0).all()   # B: > 5 m/s -> 0
            c_pts = (np.abs(g["x"] - 2.6) < 1e-3) & dyn_g
            if f == 1:
                assert (g["nx"][c_pts] < -100).all()                 # C: 30 -> 160 points: gate, unmatched
            else:
                assert np.allclose(g["ny"][c_pts], 0.0, atol=1e-3)   # 160 -> 160: matched, at rest
        o.get_occupancy_with_future(0.2); m.getOccupancyMapWithFutureStatus(0.2)
    o.close(); m.close()


def test_particle_csv_of_update(dsp, orc, tmp_path):
    """setParticleRecordFlag (:375-378) arms the CSV dump at the end of update() (:326-350): the drop-in class writes
    <folder>/particles_update_t_<counter>_<ms>.csv with the reference's columns flag,vx,vy,vz,px,py,pz,weight,voxel in
    voxel/slot order; checked against the oracle's particle array after the same frames"""
    exe = str(tmp_path / "csv_driver")
    subprocess.check_call(["g++", "-std=c++14", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csv_driver.cpp"),
                           "-L" + os.path.join(ROOT, "dsp-map_amd", "lib"), "-ldspmap_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "dsp-map_amd", "lib"), "-o", exe])
    p, v, r = common.tables(1)
    pts = common.wall_cloud(3, n_side=40, dist=2.2, half_w=1.8, half_h=0.9)
    frames = [(pts, (0.01 * f, 0.0, 0.0), f * 0.4, (1.0, 0.0, 0.0, 0.0)) for f in range(4)]
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as fh:
        np.array([len(frames), p.size, r.size], np.int32).tofile(fh)
        p.tofile(fh); v.tofile(fh); r.tofile(fh)
        for c, pos, t, q in frames:
            np.array([len(c)], np.int32).tofile(fh); np.array(pos, np.float32).tofile(fh)
            np.array([t], np.float64).tofile(fh); np.array(q, np.float32).tofile(fh); c.astype(np.float32).tofile(fh)
    out_all = tmp_path / "all"; out_all.mkdir()
    subprocess.check_call([exe, path, str(out_all), "-1", "1.0"])
    files = sorted(os.listdir(out_all))
    # negative flag: one file per frame; names carry update_counter and (int)(update_time * 1000) (:333)
    assert files == ["particles_update_t_1_0.csv", "particles_update_t_2_400.csv", "particles_update_t_3_800.csv",
                     "particles_update_t_4_1200.csv"], files
    o = orc.Oracle(orc.make_config())
    o.set_tables(p, v, r)
    o.L.dspo_use_velocity_estimator(o.h, 2)
    assert o.update(pts, frames[0][1], frames[0][2], frames[0][3]) == 1
    vo, so, ro = o.export_sparse()
    rows = [ln.rstrip("\n").split(",") for ln in open(out_all / files[0])]
    assert len(rows) == len(vo) > 5000 and all(len(x) == 9 for x in rows)
    fmt = lambda x: "%g" % x                                            # ostream << float: 6 significant digits
    assert [int(x[8]) for x in rows] == vo.tolist()                     # voxel order of the reference's loops (:337-338)
    assert all(x[0] == "1" for x in rows) and set(np.unique(ro[:, 0]).tolist()) <= {1.0, np.float32(0.6)}   # copies (0.6) are exported as live (1)
    # voxels with fewer than 5 particles are not resampled (:986): their rows equal the oracle's, column by column
    cnt = np.bincount(vo, minlength=o.V)
    small = np.nonzero(cnt[vo] < 5)[0]
    assert len(small) > 500
    for k in small:
        assert [rows[k][c] for c in range(1, 7)] == [fmt(ro[k][c]) for c in range(1, 7)], k
        assert float(rows[k][7]) == pytest.approx(float(ro[k][7]), rel=1e-4)
    # positive flag: once, the first frame whose update_time exceeds record_time (:329)
    out_once = tmp_path / "once"; out_once.mkdir()
    subprocess.check_call([exe, path, str(out_once), "1", "0.5"])
    assert sorted(os.listdir(out_once)) == ["particles_update_t_3_800.csv"]
    o.close()


def test_device_estimator_on_the_depth_stream(dsp, orc):
    """the benchmark's synthetic depth stream (corridor with ground, walls, boxes and walking pedestrians, ~5000 points
    per frame) through the device velocity estimator: birth cloud == the oracle's restatement of
    velocityEstimationThread (:1377-1544), frame after frame -- incl. a frame whose view is empty (the previous output
    is kept, :1379-1381) -- through the host-buffer call, and the captured device-resident frame ends in the same map"""
    import torch
    scene_mod = __import__("dsp-map_amd.scene", fromlist=["CorridorScene"])
    cfgkw = dict(nx=66, ny=66, nz=40, res=0.15, ppv=24)
    o, m = make_pair(dsp, orc, seed=5, **cfgkw)
    md = dsp.DSPMap(dsp.make_config(**cfgkw)); md.set_tables(*common.tables(5))
    for x in (m, md):
        x.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    o.L.dspo_use_velocity_estimator(o.h, 1)
    sc = scene_mod.CorridorScene(66 * 0.15, 66 * 0.15, 40 * 0.15, seed=1234, device="cuda")
    n_dyn_seen = 0
    for f in range(8):
        t = f / 30.0
        pts_t, pos, quat = sc.frame(t)
        if f == 5:
            pts_t = pts_t.clone(); pts_t[:, 0] *= -1.0          # everything behind the sensor: an empty view
        pts = pts_t.cpu().numpy()
        assert o.update(pts, pos, t, quat) == 1
        assert m.update(pts, pos, t, quat) == 1
        assert md.update_device(pts_t.data_ptr(), len(pts), pos, t, quat) == 1
        g, w = m.get_birth_cloud(), o.get_birth_cloud()
        assert len(g) == len(w) > 1000, f
        for k in ("x", "y", "z", "nx", "ny", "nz", "intensity"):
            assert np.array_equal(g[k], w[k]), (f, k)
        assert o.cursors()[0] == m.cursors()[0] and o.cursors()[2] == m.cursors()[2], f
        n_dyn_seen += int((g["intensity"] > 0.01).sum())
        occ_o, occ_g = o.results[:, 0].astype(np.float64), m.results()[:, 0].astype(np.float64)
        # (the empty-view frame multiplies every weight in view by 1 - P_d: particles near the 1e-3 cull threshold make the
        # mass comparison of two trajectories that already differ by resampling ties coarser from there on)
        assert abs(occ_g.sum() - occ_o.sum()) < (5e-3 if f < 5 else 2e-2) * occ_o.sum(), f
        o.get_occupancy_with_future(0.2); m.getOccupancyMapWithFutureStatus(0.2); md.getOccupancyMapWithFutureStatus(0.2)
    assert n_dyn_seen > 200                                     # the pedestrians / boxes were tagged possibly dynamic
    for a, b in zip(m.export_state(), md.export_state()):
        assert np.array_equal(a, b)                             # captured frame == host-buffer frame, slot for slot
    # moving particles exist (newborns of matched clusters carry the estimated velocity)
    rec = m.export_state()[2]
    assert (np.abs(rec[:, 1]) + np.abs(rec[:, 2]) > 0.3).sum() > 100
    o.close(); m.close(); md.close()


@pytest.mark.parametrize("est,quat", [(0, (1.0, 0.0, 0.0, 0.0)), (2, (0.9659258, 0.0, 0.0, 0.258819)), (0, (0.9238795, 0.0, 0.3826834, 0.0))])
def test_split_placement_changes_nothing(dsp, est, quat):
    """Large maps give the arrivals of the tiles that cannot see the field of view their slots on a side stream, beside the
    pair kernels (k_predict's conservative box test decides per tile; DSPMAP_P_PLACE_SPLIT_TILES).  Forced on for a small map
    and compared with the single-stream frame: every slot, every float and every counter equal -- with the sensor looking
    along x, yawed by 30 degrees (with the device estimator's branch sharing the side stream), and pitched by 45 degrees --
    and some tiles really are placed on each side."""
    import torch
    cfg = dict(nx=56, ny=88, nz=12, res=0.15, ppv=24)   # tiles straddle two rows; rows beyond the view's width exist
    tables = common.tables(5)
    maps = []
    # (DSPMAP_P_SIDE_PLACEMENT: the side launch leaving the main chain behind the list preparation (default), behind the placement of the
    # tiles with a view, behind the prediction; with one and with five workgroups per compute unit)
    for split, side in ((1, None), (2_000_000_000, None), (1, 16 + 5), (1, 32 + 1)):
        m = dsp.DSPMap(dsp.make_config(**cfg)); m.set_tables(*tables)
        m.L.dspmap_init_device(m.h)
        m.set_param(dsp.capi.P_PLACE_SPLIT_TILES, split)
        if side is not None:
            m.set_param(dsp.capi.P_SIDE_PLACEMENT, side)
            assert m.get_param(dsp.capi.P_SIDE_PLACEMENT) == side
        if est:
            m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, est)
        maps.append(m)
    for m in maps:   # (sparse: the lists stay short -- test_gpu_list_capacity.py covers lists far past their capacity)
        m.seed_uniform(2, 0.01, 11, 0.0)
    rng = np.random.default_rng(3)
    ys, zs = np.meshgrid(np.linspace(-2.0, 2.0, 41), np.linspace(-0.9, 0.9, 19))
    base = np.stack([np.full(ys.size, 2.3) + 0.2 * np.sin(2 * ys.ravel()), ys.ravel(), zs.ravel()], 1).astype(np.float32)
    moved = 0
    for f in range(6):
        t = f / 30.0
        pts = torch.from_numpy(base + rng.normal(0, 0.004, base.shape).astype(np.float32)).cuda()
        pos = (0.9 * t, 0.5 * t, 0.1 * np.sin(5 * t))
        for m in maps:
            assert m.update_device(pts.data_ptr(), len(base), pos, t, quat) == 1
            m.clearOccupancyMapPrediction()
        ca = maps[0].counters(); ca.pop("update_ms")
        for mb in maps[1:]:
            cb = mb.counters(); cb.pop("update_ms")
            assert ca == cb, (f, ca, cb)
        moved += ca["n_moved"]
    assert moved > 20000
    for mb in maps[1:]:
        for a, b in zip(maps[0].export_state(), mb.export_state()):
            assert np.array_equal(a, b)
        assert np.array_equal(maps[0].results(), mb.results())
    got = maps[0].debug_tile_fov()
    assert 0 < got.sum() < len(got), got.sum()      # both launches had tiles to place
    for m in maps:
        m.close()


def test_parameter_ring_wraps_and_empty_tiles_come_back(dsp):
    """2 300 replayed frames on a small map -- more than twice the 1 024 slots of the pinned parameter ring the captured
    frame reads its per-frame values from (the slots' guard events get used) -- against the same frames through direct
    launches (DSPMAP_P_USE_GRAPH = 0: the parameter block is copied, no ring): every slot, float and counter equal at
    the end.  The sensor looks at a wall, steps 5 m aside and receives empty clouds for 250 frames (the map runs empty: its
    tiles are skipped by the sweeps) and looks at a wall again (the tiles must be visited again), twice; the device
    estimator's branch is on."""
    import torch
    cfg = dict(nx=24, ny=24, nz=10, res=0.15, ppv=9)
    tables = common.tables(11)
    maps = []
    for graph in (1, 0):
        m = dsp.DSPMap(dsp.make_config(**cfg)); m.set_tables(*tables)
        m.L.dspmap_init_device(m.h)
        m.set_param(dsp.capi.P_USE_GRAPH, graph)
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
        maps.append(m)
    rng = np.random.default_rng(8)
    ys, zs = np.meshgrid(np.linspace(-0.9, 0.9, 13), np.linspace(-0.4, 0.4, 7))
    base = np.stack([np.full(ys.size, 1.2), ys.ravel(), zs.ravel()], 1).astype(np.float32)
    away = (0.0, 0.0, 0.0, 1.0)      # looking along -x: nothing in view
    front = (1.0, 0.0, 0.0, 0.0)
    clouds = [torch.from_numpy(base + rng.normal(0, 0.003, base.shape).astype(np.float32)).cuda() for _ in range(16)]
    live = []
    for f in range(2300):
        t = f / 30.0
        blind = 600 <= f < 850 or 1700 <= f < 1950
        q = away if blind else front
        pts = clouds[f % 16]
        hop = 5.0 * ((f >= 600) + (f >= 1700))   # a 5 m side step: every particle leaves the 3.6 m map
        pos = (0.05 * np.sin(0.7 * t), hop, 0.03 * np.sin(2.0 * t))
        for m in maps:
            assert m.update_device(pts.data_ptr(), 0 if blind else len(base), pos, t, q) == 1
            m.clearOccupancyMapPrediction()
        if f in (599, 849, 1200, 1949, 2299):
            ca, cb = maps[0].counters(), maps[1].counters()
            ca.pop("update_ms"); cb.pop("update_ms")
            assert ca == cb, (f, ca, cb)
            live.append(ca["n_live_out"])
    assert live[0] > 500 and live[2] > 500 and live[4] > 500, live     # a map at the wall ...
    assert live[1] == 0 and live[3] == 0, live                         # ... that is empty after the side step
    for a, b in zip(maps[0].export_state(), maps[1].export_state()):
        assert np.array_equal(a, b)
    assert np.array_equal(maps[0].results(), maps[1].results())
    for m in maps:
        m.close()
