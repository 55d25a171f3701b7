"""Pyramid lists far past what a list holds before its cut (run with `-m gpu` on an MI355X).

The reference registers at most SAFE_PARTICLE_NUM_PYRAMID (CAPP) particles per pyramid, in the order of its voxel / slot
sweep, and removes every later one (-2, :1245-1259).  A HIP list accepts CAPA = 2 CAPP + 64 entries before the cut
(k_pyr_prepare keeps the CAPP smallest sweep keys); the candidates beyond CAPA go to a spill pool and are cut by the same
keys.  These maps put thousands of candidates into the fullest lists -- 1.4 to 1.9 x CAPA -- and every test first proves, from
the DEVICE's own counts, that it reached that regime."""
import numpy as np
import pytest
import torch

from tests import common
from tests.test_gpu_parity import RTOL, gpu_state, make_pair
from tests.test_gpu_round2 import _slots_equal

pytestmark = pytest.mark.gpu

MAP = dict(ny=40, nz=16, res=0.15, ppv=24)
# (nx, angle): 448 pyramids (k_predict's LDS-histogram registration) / 4032 pyramids (its batch_append registration)
STAGE_MAPS = {"a3": (160, 3), "a1": (160, 1)}
PER_VOXEL = 12
EMPTY = np.zeros((0, 3), np.float32)


def _fill(o, m, seed, vmax=0.0):
    px, py, pz, vx, vy, w = common.uniform_per_voxel(o.cfg, PER_VOXEL, seed, vmax=vmax)
    return common.inject_both(o, m, px, py, pz, vx, vy, w)


def _past_capa(m):
    """pyramid lists of the last prediction with more candidates than a list holds before its cut, by the device's count"""
    return int((m.pyramid_candidates() > common.capa(m.capp)).sum())


def _check_stage(o, m, step):
    cand_o, cand_g = o.pyramid_candidates.copy(), m.pyramid_candidates()
    assert np.array_equal(cand_o, cand_g), step
    len_o = (o.pyramid_lists[:, :, 0] != 0).sum(1)
    assert np.array_equal(len_o, m.pyramid_counts()), (step, np.nonzero(len_o != m.pyramid_counts())[0][:10])
    c = m.counters()
    removed_o = int(np.maximum(cand_o - o.capp, 0).sum())
    assert c["n_pyramid_full"] == removed_o, (step, c["n_pyramid_full"], removed_o)
    assert c["n_overflow_inexact"] == 0 and c["n_voxel_full"] == 0, (step, c)
    _slots_equal(o, m, cols=(1, 2, 4, 5, 6, 7))   # the same particles in the same slots, every float
    return c


@pytest.mark.parametrize("tiling", [0, 1])
@pytest.mark.parametrize("name", list(STAGE_MAPS))
def test_stayers_past_list_capacity_against_oracle(dsp, orc, name, tiling):
    """nobody moves: the candidates of a pyramid are the particles in it, 2 to 4 x CAPA in the fullest lists.  Two
    predictions: the first cuts, the second finds the survivors only.  Lists, removals and slots equal the oracle's."""
    nx, angle = STAGE_MAPS[name]
    o, m = make_pair(dsp, orc, nx=nx, angle=angle, **MAP)
    m.set_param(dsp.capi.P_TILING, tiling)
    n = _fill(o, m, 5)
    assert n == PER_VOXEL * o.V
    for step in range(2):
        o.bin_points(EMPTY); m.bin_points(EMPTY)
        o.predict(0.0, 0.0, 0.0, 0.0); m.predict(0.0, 0.0, 0.0, 0.0)
        if step == 0:
            assert _past_capa(m) >= 20, _past_capa(m)
            assert m.get_param(dsp.capi.P_TILING) == tiling
        c = _check_stage(o, m, step)
        if step == 0:
            assert c["n_pyramid_full"] > 100000, c
    o.close(); m.close()


@pytest.mark.parametrize("tiling", [0, 1])
@pytest.mark.parametrize("name", list(STAGE_MAPS))
def test_movers_past_list_capacity_against_oracle(dsp, orc, name, tiling):
    """every particle moving (+-1.5 m/s) and a sensor shift: k_place's arrivals compete with the stayers for lists that are
    past CAPA already; the slots that turned-away particles hand back go to the arrivals behind them in the sweep"""
    nx, angle = STAGE_MAPS[name]
    o, m = make_pair(dsp, orc, nx=nx, angle=angle, **MAP)
    m.set_param(dsp.capi.P_TILING, tiling)
    _fill(o, m, 6, vmax=1.5)
    o.bin_points(EMPTY); m.bin_points(EMPTY)
    reslotted = 0
    for step, st in enumerate([(-0.03, 0.02, 0.0, 0.1), (0.02, -0.01, 0.0, 0.1)]):
        o.predict(*st); m.predict(*st)
        if step == 0:
            assert _past_capa(m) >= 20, _past_capa(m)
        c = _check_stage(o, m, step)
        assert c["n_moved"] > 100000, c
        reslotted += c["n_reslotted"]
        # the frame's resampling on both sides (bit-exact from the same state): a moved particle is predicted again only after
        # it (:649,968)
        o.occupancy_resample(); m.occupancy_resample()
        o.L.dspo_clear_future(o.h); m.clearOccupancyMapPrediction()
    assert reslotted > 0
    o.close(); m.close()


@pytest.mark.parametrize("split", [0, 1])
def test_whole_frames_past_list_capacity_against_oracle(dsp, orc, split):
    """two captured frames (update_device) from a state whose lists are far past CAPA, against the oracle's update(): the
    bars of test_full_size_config_c_whole_frame_against_oracle; the first frame's removals equal the oracle's, the later ones'
    to 0.1 %"""
    o, m = make_pair(dsp, orc, seed=3, nx=160, angle=3, **MAP)
    if split:
        m.set_param(dsp.capi.P_PLACE_SPLIT_TILES, 1)
    o.L.dspo_use_velocity_estimator(o.h, 1)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    _fill(o, m, 7, vmax=0.5)
    pts = common.wall_cloud(7, n_side=48, dist=7.0, half_w=2.6, half_h=1.0)
    d = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    for f in range(2):
        pos, t = (0.02 * f, -0.01 * f, 0.0), f / 30.0
        assert o.update(pts, pos, t, (1, 0, 0, 0)) == 1
        assert m.update_device(d.data_ptr(), len(pts), pos, t, (1, 0, 0, 0)) == 1
        if f == 0:
            assert _past_capa(m) >= 20, _past_capa(m)
        removed_o = int(np.maximum(o.pyramid_candidates - o.capp, 0).sum())
        c = m.counters()
        if f == 0:
            assert c["n_pyramid_full"] == removed_o, (f, c["n_pyramid_full"], removed_o)
        else:
            # (after a resampling the two states may differ in the voxels with equal-weight threshold ties, DESIGN.md "Numerics":
            # the later frames' removals are held to the live-count bar)
            assert abs(c["n_pyramid_full"] - removed_o) <= 1e-3 * removed_o, (f, c["n_pyramid_full"], removed_o)
        occ_o, occ_g = o.results[:, 0], m.results()[:, 0]
        err = np.abs(occ_g - occ_o)
        tol = RTOL * np.maximum(1.0, np.abs(occ_o))
        assert (err <= tol).mean() > 0.999, (f, (err > tol).sum())
        assert abs(occ_g.astype(np.float64).sum() - occ_o.astype(np.float64).sum()) < 1e-4 * occ_o.sum(), f
        live_o = o.L.dspo_count_live(o.h)
        assert abs(c["n_live_out"] - live_o) < 1e-3 * live_o, (f, c["n_live_out"], live_o)
        xo, fo = o.get_occupancy_with_future(0.2)
        ng, xg, fg = m.getOccupancyMapWithFutureStatus(0.2)
        assert np.allclose(fg.sum(0), fo.sum(0), rtol=5e-3), f
    assert removed_o >= 0 and c["n_born"] > 1000
    o.close(); m.close()


def test_alternating_sweep_direction_past_list_capacity_changes_nothing(dsp):
    """test_alternating_sweep_direction_changes_nothing with the lists far past CAPA: a reversed sweep delivers the largest
    sweep keys first, so a list that dropped entries in arrival order would keep other particles"""
    from tests.test_gpu_round4 import _alternating_sweep
    past = _alternating_sweep(dsp, 20)
    assert past[0] >= 20, past


def test_identical_maps_past_list_capacity_are_identical(dsp):
    """three maps seeded alike far past CAPA and fed six identical frames: every slot, float and counter equal after every
    frame -- which particles a full list keeps does not depend on the order in which the workgroups arrive"""
    cfg = dict(nx=160, angle=3, **MAP)
    tables = common.tables(8)
    maps = []
    for _ in range(3):
        m = dsp.DSPMap(dsp.make_config(**cfg)); m.set_tables(*tables)
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
        m.seed_uniform(PER_VOXEL, 0.01, 31, 1.0)
        maps.append(m)
    pts = common.wall_cloud(5, n_side=48, dist=7.0, half_w=2.6, half_h=1.0)
    d = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    past = []
    for f in range(6):
        pos, t = (0.03 * f, 0.01 * f, 0.0), f / 30.0
        for m in maps:
            assert m.update_device(d.data_ptr(), len(pts), pos, t, (1.0, 0.0, 0.0, 0.0)) == 1
        past.append(_past_capa(maps[0]))
        cs = [m.counters() for m in maps]
        for c in cs:
            c.pop("update_ms")
        assert cs[0] == cs[1] == cs[2], (f, cs)
        futs = [m.getFutureStatus() for m in maps]
        assert np.array_equal(futs[0], futs[1]) and np.array_equal(futs[0], futs[2]), f
        for m in maps[1:]:
            for a, b in zip(maps[0].export_state(), m.export_state()):
                assert np.array_equal(a, b), f
            assert np.array_equal(maps[0].results(), m.results()), f
    assert past[0] >= 20, past
    for m in maps:
        m.close()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_map_past_list_capacity_is_the_unsharded_map(dsp, world):
    """_sharded_overfull on a map whose lists are past CAPA on the unsharded map and in the slabs: with exact lists (the
    distributed selection of the CAPP-th smallest key over all ranks) the sharded map is the unsharded one, bit for bit"""
    from tests.test_gpu_round4 import _sharded_overfull
    same, stats, inexact = _sharded_overfull(dsp, world, exact=True, nx=160, per_voxel=12)
    assert stats[0][5] >= 20, stats                               # the unsharded map's lists past CAPA
    if world == 2:
        assert max(s[6] for s in stats) > 0, stats                # ... and a slab's own share of a list
    assert stats[0][0] > 100000 and all(s[0] > 200 for s in stats), stats   # every frame turned particles away
    assert same, (stats, inexact)
