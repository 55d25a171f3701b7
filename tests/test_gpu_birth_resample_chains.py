"""GPU parity tests (run with `-m gpu`) for the parts of the birth kernels whose load chains were shortened, and for the cases
that the same kind of change in k_resample_wg has to get right (tried, measured slower, not in the tree: LOG.md):

  * k_birth_insert<FUSED>'s cursor prefix -- a block-wide exclusive scan over the window of per-point draw counts instead of a
    per-thread serial walk -- through both frames that reach the fused insertion (a caller-supplied dynamic birth cloud; the
    device velocity estimator), over the newborn numbers and cloud lengths at which the window, the groups of 16 points and the
    blocks of 256 children fall differently;
  * the wave-aggregated bucket atomics of the newborn children (birth_child_thread, birth_point_wave): groups that straddle the
    bucket capacity and the overflow list, groups of one lane, children outside the map;
  * k_resample_wg<1> / <2>: many copies of a late survivor into slots freed before it, a full voxel, voxels at the resampling
    threshold, tiles whose only moving entries sit either side of wave 1's step of eight entries, tiles without a moving entry.

All against the CPU oracle.  Bars: slots, positions, velocities, cursors, per-voxel mass and mean velocity bit-exact; weights
after a weight update rel 1e-4 (tests/test_gpu_parity.py); future status 1e-4.

Why the frame tests start from an EMPTY map with sources two voxels apart and 32 particles per voxel: a frame ends with the
resampling, whose keep / remove thresholds compare sums of weights that agree with the oracle's to 1e-4 only (the newborn
weight is nb_weight * sum 1/Ck).  With at most one source per voxel (<= 32 children = M) every voxel keeps all its particles
with a margin of half a weight, so the state after the frame IS the newborns, and the comparison can be exact.  The pre-birth
occupancy, full voxels and the overflow list are exercised through the birth STAGE, which has no resampling behind it."""
import numpy as np
import pytest

from tests import common
from tests.test_gpu_configs import _slot_exact
from tests.test_gpu_parity import gpu_state
from tests.test_gpu_round4 import _check_resample, _force

pytestmark = pytest.mark.gpu

RES = 0.15


def _pair(dsp, orc, seed, sigma_p=0.05, **cfgkw):
    o = orc.Oracle(orc.make_config(**cfgkw))
    m = dsp.DSPMap(dsp.make_config(**cfgkw))
    p, v, r = common.tables(seed, sigma_p=sigma_p)
    o.set_tables(p, v, r)
    m.set_tables(p, v, r)
    return o, m


def _set_nb(o, m, nb):
    o.L.dspo_set_newborn_number(o.h, nb)
    m.setNewBornParticleNumberofEachPoint(nb)


def _centre(cfg, ix, iy, iz):
    hx, hy, hz = common.half_extent(cfg)
    return np.array([-hx + (ix + 0.5) * RES, -hy + (iy + 0.5) * RES, -hz + (iz + 0.5) * RES], np.float64)


def _voxel_index(cfg, ix, iy, iz):
    return (iz * cfg.ny + iy) * cfg.nx + ix


# ---------------------------------------------------------------------------------------------------------------------------
# cursor prefix
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("matched", "outside", "static", "unmatched", "faint")   # by index i % 5: zero entries of birth_cvr between non-zero ones


def _mixed_sources(orc, cfg, n, seed):
    """n birth sources: matched (velocity-table draws), outside the map (no source at all), static (intensity 0: children, no
    draws), unmatched (rand() draws), faint (tagged, but intensity <= 0.01: no draws) -- interleaved; the sources inside the
    map sit at the centres of distinct voxels two apart on every axis"""
    rng = np.random.default_rng(seed)
    cells = [(ix, iy, iz) for iz in range(0, cfg.nz, 2) for iy in range(0, cfg.ny, 2) for ix in range(0, cfg.nx, 2)]
    order = rng.permutation(len(cells))
    src = np.zeros(n, orc.VPOINT_DTYPE)
    used = 0
    for i in range(n):
        kind = KINDS[i % 5]
        if kind == "outside":
            p = np.array([5.0 + 0.01 * i, 0.3, 0.1])
        else:
            p = _centre(cfg, *cells[order[used]])
            used += 1
        src["x"][i], src["y"][i], src["z"][i] = p
        if kind in ("matched", "outside", "faint"):
            src["nx"][i], src["ny"][i] = rng.uniform(-1, 1, 2)
        if kind == "unmatched":
            src["nx"][i] = src["ny"][i] = src["nz"][i] = -10000
        src["intensity"][i] = {"matched": 0.6, "outside": 0.7, "static": 0.0, "unmatched": 0.4, "faint": 0.005}[kind]
    assert used <= len(cells)
    return src


@pytest.mark.parametrize("n_birth", [1, 16, 17, 33, 600])
@pytest.mark.parametrize("nb", [1, 7, 20, 32])
def test_fused_cursor_prefix_with_caller_supplied_cloud(dsp, orc, nb, n_birth):
    """dspmap_update_device with a device-resident dynamic birth cloud (children on k_place's launch, k_birth_split_cksum_cvr<false>,
    k_birth_insert<true>) against the oracle's update() with the same cloud: after the frame every particle -- the newborns --
    sits in the same slot with the same position and velocity bits, and the three stream cursors are equal.
    nb = 1: a block spans 256 points (the longest window, 16 groups of 16); 7: points straddle waves and blocks; 20: the default;
    32: the width of the `inside` word.  n_birth 1 / 16 / 17 / 33 / 600: edges of the groups of 16 and (with nb) of the blocks."""
    import torch
    cfgkw = dict(nx=24, ny=24, nz=8, res=RES, ppv=32)
    o, m = _pair(dsp, orc, 21, **cfgkw)
    _set_nb(o, m, nb)
    o.L.dspo_use_velocity_estimator(o.h, 0)
    pts = common.wall_cloud(13, n_side=20, dist=1.2, half_w=0.9, half_h=0.4)
    src = _mixed_sources(orc, o.cfg, n_birth, 100 + n_birth)
    pos = (0.0, 0.0, 0.0)
    d_pts = torch.from_numpy(pts).cuda()
    d_src = torch.from_numpy(src.view(np.float32).reshape(-1, 7).copy()).cuda()
    o.set_birth_cloud(src)
    assert o.update(pts, pos, 0.0, (1, 0, 0, 0)) == 1
    assert m.update_device(d_pts.data_ptr(), len(pts), pos, 0.0, (1, 0, 0, 0), birth_dev_ptr=d_src.data_ptr(), n_birth=len(src)) == 1
    assert o.cursors() == m.cursors()
    vo, so, ro, rg = _slot_exact(o, m, cols=(1, 2, 4, 5, 6))
    assert np.allclose(ro[:, 7], rg[:, 7], rtol=1e-4)
    n_src = sum(1 for i in range(n_birth) if KINDS[i % 5] != "outside")
    assert 0.5 * n_src * nb < len(vo) <= n_src * nb                     # most children are inside the map and alive
    if n_birth >= 16 and nb >= 7:
        assert ((ro[:, 1] != 0) | (ro[:, 2] != 0)).sum() >= 2           # both drawing branches left moving newborns
    assert m.counters()["n_born"] == len(vo)
    o.close(); m.close()


def _estimator_scene(t, frame):
    """sensor-frame cloud for a 24x24x8 map around a sensor 0.45 m above the ground: a ground strip (static sources: zero
    entries), a cluster beyond the map's edge (the largest: first in the cloud, not a source), a cluster moving at 1 m/s
    (unmatched in frame 0: rand() draws; matched in frame 1: velocity-table draws), one that appears in frame 1 (unmatched)
    and a group below the minimum size.  Points are one voxel (0.15 m) apart on planes: one source per voxel."""
    def box(x0, y0, z0, nx, ny, nz, step=0.15):
        xs, ys, zs = np.meshgrid(x0 + step * np.arange(nx), y0 + step * np.arange(ny), z0 + step * np.arange(nz), indexing="ij")
        return np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)
    parts = [box(1.2, -0.6, -0.40, 4, 9, 1),                      # ground: z_world = 0.05 <= 0.1, 36 points
             box(2.4, -0.9, -0.3, 1, 8, 5),                        # 40 points at x = 2.4: outside the map (half extent 1.8)
             box(1.2, -0.5 + 1.0 * t, -0.2, 1, 4, 5),              # 20 points, 1 m/s along +y
             box(1.5, 0.8, -0.1, 1, 1, 3)]                         # 3 points: dropped
    if frame >= 1:
        parts.append(box(1.5, 0.1, -0.1, 1, 3, 4))                 # 12 points, new in frame 1
    return np.concatenate(parts).astype(np.float32)


def _same_where_counts_agree(o, m):
    """tests/test_gpu_round4.py's comparison after a frame whose resampling saw weights that agree to 1e-4 only (thresholds may
    tie): the voxels whose particle count agrees must be nearly all, with the same slots and the same position / velocity bits"""
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    co, cg = np.bincount(vo, minlength=o.V), np.bincount(vg, minlength=o.V)
    same = co == cg
    assert same.mean() > 0.999 and abs(len(vo) - len(vg)) <= 1e-3 * len(vo) + 2
    mo, mg = same[vo[ko]], same[vg[kg]]
    assert np.array_equal(vo[ko][mo], vg[kg][mg]) and np.array_equal(so[ko][mo], sg[kg][mg])
    frac = (ro[ko][mo][:, 1:7] == rg[kg][mg][:, 1:7]).all(axis=1).mean()
    assert frac > 0.999, frac
    return ro[ko][mo]


@pytest.mark.parametrize("nb", [1, 7, 20, 32])
def test_fused_cursor_prefix_with_device_estimator(dsp, orc, nb):
    """the captured frame with the device velocity estimator (children generated by the split's waves: birth_point_wave and its
    wave-aggregated bucket atomics; k_birth_insert<true>) against the oracle's update() with its restated estimator, two frames
    from an empty map: the same birth cloud and equal cursors after every frame, and after every frame the same particles in
    the same slots with the same position and velocity bits (a voxel with more than M equal-weight newborns resamples on
    thresholds that tie exactly: the comparison is tests/test_gpu_round4.py's, on the voxels whose particle count agrees, which
    must be nearly all).
    The cloud's length is the scene's (the estimator emits it), so only nb is a parameter here.  A cloud dense enough to
    overfill a bucket (more than 128 children in a voxel) is not part of it: such a voxel holds more than M equal newborns and
    its resampling ties exactly, on this build and on its parent alike (27 points in two voxels: different survivors from frame
    0 on); the overflow list is ranked against the oracle in the birth-stage test below, through the same birth_bucket_put."""
    cfgkw = dict(nx=24, ny=24, nz=8, res=RES, ppv=32)
    o, m = _pair(dsp, orc, 22, **cfgkw)
    _set_nb(o, m, nb)
    o.L.dspo_use_velocity_estimator(o.h, 1)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    pos = (0.0, 0.0, 0.45)
    for f in range(2):
        t = f * 0.1
        pts = _estimator_scene(t, f)
        assert o.update(pts, pos, t, (1, 0, 0, 0)) == 1
        assert m.update(pts, pos, t, (1, 0, 0, 0)) == 1
        assert o.cursors() == m.cursors(), f
        g, w = m.get_birth_cloud(), o.get_birth_cloud()
        assert len(g) == len(w) >= 56 and np.array_equal(g["x"], w["x"]) and np.array_equal(g["nx"], w["nx"]), f
        rec = _same_where_counts_agree(o, m)
        if f == 0:
            assert (w["nx"] < -100).sum() >= 20 and (w["intensity"] == 0).sum() >= 36       # rand() sources and static ones
            o.get_occupancy_with_future(0.2); m.getOccupancyMapWithFutureStatus(0.2)
        else:
            assert ((w["intensity"] > 0.01) & (w["nx"] > -100) & (w["ny"] != 0)).sum() >= 20      # a matched, moving cluster
            if nb >= 7:
                assert ((rec[:, 1] != 0) | (rec[:, 2] != 0)).sum() > 20                      # moving newborns are in the map
    o.close(); m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# bucket aggregation (birth stage from an injected state: no resampling behind it)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_p", [0.005, 0.05])
def test_bucket_aggregation_against_oracle(dsp, orc, sigma_p):
    """mapAddNewBornParticlesByObservation (:796-921) through the birth stage: slot-exact against the oracle, cursors equal, the
    same number born.  sigma_p = 0.005: all 20 children of a point fall into its own voxel -- 8 points in ONE voxel make 160,
    more than a bucket holds: a wave's group straddles the capacity, the overflow list is ranked, and the voxel (5 of its 48
    slots taken) fills up.  sigma_p = 0.05: the children of a point at a voxel's corner split over several voxels, down to a
    group of one lane.  Both: points at the map's edge whose children partly fall outside."""
    cfgkw = dict(nx=16, ny=16, nz=8, res=RES, ppv=24)
    o, m = _pair(dsp, orc, 23, sigma_p=sigma_p, **cfgkw)
    cfg = o.cfg
    hx, hy, hz = common.half_extent(cfg)
    rng = np.random.default_rng(3)
    # state: 5 particles in the crowded voxel, a light background elsewhere
    c0 = _centre(cfg, 9, 5, 3)
    px, py, pz, vx, vy, w = common.random_particles(7, 3000, (hx, hy, hz), vmax=1.0, wlo=0.01, whi=0.08)
    px = np.concatenate([np.full(5, c0[0], np.float32) + 0.01 * np.arange(5, dtype=np.float32), px])
    py = np.concatenate([np.full(5, c0[1], np.float32), py]); pz = np.concatenate([np.full(5, c0[2], np.float32), pz])
    vx = np.concatenate([np.zeros(5, np.float32), vx]); vy = np.concatenate([np.zeros(5, np.float32), vy])
    w = np.concatenate([np.full(5, 0.03, np.float32), w])
    common.inject_both(o, m, px, py, pz, vx, vy, w)
    pts = common.wall_cloud(5, n_side=20, dist=0.9, half_w=0.7, half_h=0.35)
    cur = (0.0, 0.0, 0.0)
    for x in (o, m):
        x.set_current_position(*cur) if x is m else x.L.dspo_set_current_position(x.h, *cur)
        x.bin_points(pts, (1, 0, 0, 0))
        x.predict(0, 0, 0, 0)
        x.map_update()
    crowd = c0 + rng.uniform(-0.02, 0.02, (8, 3))                                            # 8 points in ONE voxel
    corner = np.array([_centre(cfg, 4, 4, 2) + 0.5 * RES - 0.004, _centre(cfg, 11, 10, 5) + [0.5 * RES - 0.002, 0.0, 0.03],
                       _centre(cfg, 3, 12, 4) + [0.06, -0.07, 0.072]])                       # corners / faces of voxels
    edge = np.array([[hx - 0.01, 0.2, 0.1], [-hx + 0.004, -0.5, 0.2], [0.3, hy - 0.02, -hz + 0.01], [0.1, -0.2, hz - 0.003]])
    spread = np.stack([rng.uniform(-0.9 * hx, 0.9 * hx, 40), rng.uniform(-0.9 * hy, 0.9 * hy, 40), rng.uniform(-0.9 * hz, 0.9 * hz, 40)], 1)
    p = np.concatenate([crowd[:4], corner, edge, crowd[4:], spread])                         # (the crowd is not contiguous in the cloud)
    src = np.zeros(len(p), orc.VPOINT_DTYPE)
    src["x"], src["y"], src["z"] = p[:, 0], p[:, 1], p[:, 2]
    dyn = np.arange(0, len(p), 2)
    src["intensity"][dyn] = rng.uniform(0.1, 1.0, len(dyn))
    src["nx"][dyn] = rng.uniform(-1, 1, len(dyn)); src["ny"][dyn] = rng.uniform(-1, 1, len(dyn))
    src["nx"][dyn[::3]] = -10000; src["ny"][dyn[::3]] = -10000; src["nz"][dyn[::3]] = -10000
    o.L.dspo_use_velocity_estimator(o.h, 0)
    o.set_birth_cloud(src); m.set_birth_cloud(src)
    o.add_newborn(); m.add_newborn()
    assert o.cursors() == m.cursors()
    vo, so, ro, rg = _slot_exact(o, m, cols=(0, 1, 2, 4, 5, 6))
    assert np.allclose(ro[:, 7], rg[:, 7], rtol=1e-4)
    c = m.counters()
    newborn = ro[:, 0] > 10
    assert c["n_born"] == int(newborn.sum()) > 500
    v0 = _voxel_index(cfg, 9, 5, 3)
    if sigma_p < 0.01:
        assert (vo == v0).sum() == o.slots and c["n_born_dropped"] >= 160 - (o.slots - 5)    # the crowded voxel filled up, in rank order
    else:
        per_point_voxels = [len(np.unique(vo[newborn & (np.abs(ro[:, 4] - q[0]) < 0.2) & (np.abs(ro[:, 5] - q[1]) < 0.2)])) for q in corner]
        assert max(per_point_voxels) >= 3                                                     # children of one point in three voxels or more
    assert c["n_born"] + c["n_born_dropped"] < 20 * len(p)                                    # some children fell outside the map
    o.close(); m.close()


# ---------------------------------------------------------------------------------------------------------------------------
# k_resample_wg: copies into freed slots, moving entries either side of wave 1's step
# ---------------------------------------------------------------------------------------------------------------------------
def _resample_cases(cfg):
    """particles of the cases, each in a voxel (and tile) of its own, + a static background: returns the arrays for
    inject_both, the list of case voxels and a dict of named voxels"""
    rng = np.random.default_rng(17)
    recs = []      # (ix, iy, iz, vx, vy, w, flag)
    named = {}

    def put(name, cell, vel, wts, flags=None):
        named[name] = cell
        for j, wj in enumerate(wts):
            recs.append(cell + (vel[j][0], vel[j][1], wj, 1.0 if flags is None else flags[j]))

    Z = (0.0, 0.0)
    # 30 survivors, the one in slot 25 carries 90 % of the weight (and moves): many copies, into slots freed by survivors removed before it
    wts = [0.01] * 30; wts[25] = 9 * 0.29
    put("heavy_late", (9, 1, 1), [Z] * 25 + [(0.5, -0.3)] + [Z] * 4, wts)
    # a full voxel: the heavy early particles cannot be copied, their weight is folded back (:1037-1041)
    named["_full_cell"] = (9, 5, 1)
    # exactly 4 survivors (no resampling) and exactly 5 (the smallest voxel that is resampled), one culled particle (w < 1e-3) between them
    put("four", (9, 9, 1), [Z, (0.2, 0.1), Z, Z, Z], [0.03, 0.05, 0.0005, 0.02, 0.04])
    put("five", (9, 13, 1), [Z, Z, (0.2, 0.1), Z, Z, Z], [0.03, 0.0004, 0.05, 0.02, 0.04, 0.2])
    # tiles whose only moving entries are entries 7 / 8 of a voxel (either side of wave 1's step of eight); a culled particle in slot 2
    # makes entry j sit in slot j + 1
    for name, cell, mv in (("entries_7_8", (13, 1, 5), (7, 8)), ("entry_7", (13, 5, 5), (7,)), ("entry_8", (13, 9, 5), (8,))):
        wts = list(rng.uniform(0.02, 0.06, 12)); wts[2] = 0.0005
        vel = [Z] * 12
        for e in mv:
            vel[e + 1] = (0.4, 0.25)
        put(name, cell, vel, wts)
    # moving newborns (flag 15) beside static old particles
    put("newborns", (13, 13, 5), [(0.6, -0.2) if j % 2 else Z for j in range(10)], list(rng.uniform(0.02, 0.2, 10)), [15.0 if j % 2 else 1.0 for j in range(10)])
    return recs, named


@pytest.mark.parametrize("variant", ["wg+inline", "wg+windows"])
@pytest.mark.parametrize("ppv", [24, 36])
def test_resample_wg_copies_and_moving_entries(dsp, orc, ppv, variant):
    """mapOccupancyCalculationAndResample (:924-1057) through the resampling stage from an injected state, k_resample_wg<1> (24
    per voxel, one occupancy word) and <2> (36 per voxel, two words) forced, with its inline rollout and with k_rollout: per-voxel
    mass and mean velocity bit-equal, survivors and copies slot-exact with equal positions and velocities, future status to 1e-4
    (tests/test_gpu_round4.py's _check_resample).  Cases, each in a tile of its own: a late heavy survivor copied into slots
    freed before it; a full voxel (fold-back); exactly 4 and exactly 5 survivors; tiles whose only moving entries are entries
    7 and / or 8 of a voxel; moving newborns beside static old particles; and a static background (tiles with no moving entry)."""
    cfgkw = dict(nx=16, ny=16, nz=8, res=RES, ppv=ppv)
    o, m = _pair(dsp, orc, 5, **cfgkw)
    want = _force(m, dsp, variant)
    cfg = o.cfg
    recs, named = _resample_cases(cfg)
    full = named.pop("_full_cell")
    wts = [0.002] * o.slots; wts[0] = 0.5; wts[5] = 0.3
    recs += [full + (0.0, 0.0, wj, 1.0) for wj in wts]
    named["full"] = full
    cells = np.array([r[:3] for r in recs])
    jit = np.random.default_rng(2).uniform(-0.04, 0.04, (len(recs), 3))
    ctr = np.array([_centre(cfg, *c) for c in cells]) + jit
    case_vox = {_voxel_index(cfg, *c) for c in named.values()}
    # static background: 4000 particles over the whole map, none in a case voxel (their counts are part of the cases)
    hx, hy, hz = common.half_extent(cfg)
    bx, by, bz, _, _, bw = common.random_particles(9, 4000, (hx, hy, hz), wlo=0.002, whi=0.05)
    bi = [np.clip(((a + h) / RES).astype(int), 0, n - 1) for a, h, n in ((bx, hx, cfg.nx), (by, hy, cfg.ny), (bz, hz, cfg.nz))]
    keep = ~np.isin(_voxel_index(cfg, *bi), list(case_vox))
    # ... and nothing static in the tiles of the "no other moving entry" cases is needed: static particles do not move
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    px = f32(np.concatenate([ctr[:, 0], bx[keep]])); py = f32(np.concatenate([ctr[:, 1], by[keep]])); pz = f32(np.concatenate([ctr[:, 2], bz[keep]]))
    vx = f32(np.concatenate([[r[3] for r in recs], np.zeros(keep.sum())])); vy = f32(np.concatenate([[r[4] for r in recs], np.zeros(keep.sum())]))
    w = f32(np.concatenate([[r[5] for r in recs], bw[keep]]))
    flag = f32(np.concatenate([[r[6] for r in recs], np.ones(keep.sum())]))
    n = common.inject_both(o, m, px, py, pz, vx, vy, w, flag)
    assert n == len(px)
    vo, so, ro = o.export_sparse()
    for name, cell in named.items():                                  # the cases are what they claim to be
        sel = vo == _voxel_index(cfg, *cell)
        exp = {"heavy_late": 30, "full": o.slots, "four": 5, "five": 6, "entries_7_8": 12, "entry_7": 12, "entry_8": 12, "newborns": 10}[name]
        assert sel.sum() == exp and np.array_equal(np.sort(so[sel]), np.arange(exp)), name
    tiles = m.tile_of(np.array([_voxel_index(cfg, *c) for c in named.values()], np.int32))
    assert len(np.unique(tiles)) == len(named)                        # one tile each
    moving = (ro[:, 1] != 0) | (ro[:, 2] != 0)
    assert len(np.unique(m.tile_of(vo[moving]))) == len(named) - 1 < len(np.unique(m.tile_of(vo)))   # ("full" is static) tiles without a moving entry exist
    o.occupancy_resample(); m.occupancy_resample()
    assert m.rollout_paths()[0] == want
    _check_resample(o, m, 6)
    vo, so, ro = o.export_sparse()
    heavy = vo == _voxel_index(cfg, *named["heavy_late"])
    assert (ro[heavy, 1] == np.float32(0.5)).sum() >= 15             # the heavy particle WAS copied many times, velocity included
    fullv = vo == _voxel_index(cfg, *named["full"])
    assert ro[fullv, 7].max() > 1.9 * ro[fullv, 7].min()             # a folded (fat) particle exists
    o.close(); m.close()
