"""The edge configurations of tests/config_edges.py without a GPU: every scene satisfies the coverage conditions it states (a later
edit of a scene cannot silently stop exercising its edge), the oracle keeps its own invariants there, dspmap_create accepts every
entry with the oracle's derived sizes, and k_rollout's window plan is the one each entry is named for."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import config_edges as E


def _oracle(orc, name, seed=1):
    o = orc.Oracle(orc.make_config(**E.EDGES[name]["cfg"]))
    o.set_tables(*common.tables(seed))
    return o


@pytest.mark.parametrize("name", list(E.EDGES))
def test_scene_meets_its_coverage_conditions(orc, name):
    kind = E.EDGES[name]["kind"]
    o = _oracle(orc, name)
    n = E.inject_edge(name, o, None)
    assert n > 0
    pts = E.observation_cloud(o.cfg)
    assert o.bin_points(pts, E.quat_of(name)) > 0
    if kind == "slots":
        before = E.check_slot_coverage(o)
        o.predict(0.05, -0.07, 0.0, 0.2)
        E.check_slot_coverage(o)                                  # the over-filled box does not move: still full
        o.occupancy_resample()
        E.check_slot_coverage(o, need_full=False)
        o2 = _oracle(orc, name)
        E.inject_edge(name, o2, None)
        o2.occupancy_resample()
        E.check_resample_coverage(o2, before)
        o2.close()
    elif kind == "tiny":
        voxel, slot, rec, per_voxel = E.slot_census(o)
        assert o.V < 64 and slot.max() == o.slots - 1 - (2 if o.V == 1 else 0) and per_voxel.max() <= o.slots
        if o.V > 1:
            assert (per_voxel == o.slots).any() and (per_voxel == 0).any()
    elif kind == "planes":
        nh, nv = E.check_plane_coverage(o)
        if name == "planes_max":
            assert (nh + 1, nv + 1) == (129, 97) and o.capp == 2
            o.predict(0.0, 0.0, 0.0, 0.0)
            assert (o.pyramid_candidates > o.capp).sum() >= 20    # in-view lists are cut ...
        else:
            assert nh * nv * o.cfg.angle_resolution ** 2 < 4 * o.cfg.half_fov_h * o.cfg.half_fov_v      # the pyramid count truncates
    elif kind == "wide":
        E.check_wide_coverage(o)
        o.predict(0.0, 0.0, 0.0, 0.0)
        E.check_lists_uncut(o)                                    # ... and on the wide grid none is (this case is about the rollout)
    else:
        E.check_slot_coverage(o)
    o.close()


def test_coverage_conditions_notice_a_scene_without_its_over_fill(orc):
    """the uniform 1.2 M per voxel that the over-filled box replaces reaches neither the last slot nor a full voxel at 64 slots"""
    o = _oracle(orc, "slots64")
    E.inject_state(o, None, over_fill=False)
    with pytest.raises(AssertionError):
        E.check_slot_coverage(o)
    o.close()


@pytest.mark.parametrize("name", list(E.EDGES))
def test_oracle_invariants_on_every_edge(orc, name):
    """bin_points -> predict -> map_update -> add_newborn -> occupancy_resample from the entry's scene: counts within the slots, every
    particle in the voxel that holds it, the resampler's mass conservation and counts, future status non-negative and T wide"""
    o = _oracle(orc, name)
    n = E.inject_edge(name, o, None, newborn_frac=0.0)
    pts = E.observation_cloud(o.cfg)
    o.L.dspo_use_velocity_estimator(o.h, 2)
    assert o.bin_points(pts, E.quat_of(name)) > 0
    o.predict(0.01, -0.02, 0.0, 1 / 30.0)
    voxel, slot, rec, per_voxel = E.slot_census(o)
    assert 0 < len(voxel) <= n and per_voxel.max() <= o.slots and slot.max() <= o.slots - 1 and not rec[:, 3].any()
    idx = C.c_int()
    for k in range(0, len(voxel), 53):
        assert o.L.dspo_voxel_index(o.h, rec[k, 4], rec[k, 5], rec[k, 6], C.byref(idx)) == 1 and idx.value == voxel[k]
    o.map_update()
    # the oracle is the yardstick of a 1e-4 bar on the newborn weight only while its own sequential fp32 normaliser is well inside it
    assert E.reference_normaliser_error(o) < 2.5e-5, E.reference_normaliser_error(o)
    w = o.export_sparse()[2][:, 7]
    assert np.isfinite(w).all() and (w >= 0).all()
    o.L.dspo_static_birth_cloud(o.h)
    o.add_newborn()
    voxel, slot, rec, per_voxel = E.slot_census(o)
    assert per_voxel.max() <= o.slots and slot.max() <= o.slots - 1 and (rec[:, 0] > 10).any()
    E.oracle_invariants_of_resample(o)
    fut = o.results[:, 4:]
    assert fut.shape == (o.V, o.T) and (fut >= 0).all()
    o.close()


@pytest.mark.parametrize("name", list(E.EDGES))
def test_create_accepts_every_edge_with_the_oracles_sizes(dsp, orc, name):
    cfg = E.EDGES[name]["cfg"]
    L = dsp.load_library()
    o = orc.Oracle(orc.make_config(**cfg))
    c = dsp.make_config(**cfg)
    h = L.dspmap_create(C.byref(c))
    assert h
    assert L.dspmap_voxel_num(h) == o.V
    assert L.dspmap_slots_per_voxel(h) == o.L.dspo_slots_per_voxel(o.h) == E.slots_of(name)
    assert L.dspmap_pyramid_num(h) == o.L.dspo_pyramid_num(o.h)
    assert L.dspmap_pyramid_capacity(h) == o.L.dspo_pyramid_capacity(o.h)
    L.dspmap_destroy(h)
    o.close()


def test_create_accepts_a_map_past_two_to_the_24_voxels(dsp):
    m = dsp.DSPMap(dsp.make_config(**E.BIG))
    assert m.V > 1 << 24 and m.V * m.slots < 1 << 31
    m.close()


def test_rollout_window_plan_of_the_edges(dsp):
    """dspmap_debug_rollout_plan (host state): t16's sixteen windows fit the LDS with halos of at least one row; the wide grid in index
    order gets the collapsed plan (every halo 0, 512 cells per horizon) -- on cubes it does not; t0 has no window"""
    def plan(name, tiling):
        m = dsp.DSPMap(dsp.make_config(**E.EDGES[name]["cfg"]))
        m.set_param(dsp.capi.P_TILING, tiling)
        out = m.rollout_plan()
        m.close()
        return out
    halo, cells = plan("t16", 0)
    assert len(halo) == 16 and min(halo) >= 1 and halo == sorted(halo) and 16 * 512 < cells <= 30000
    assert cells == sum(512 + 2 * h * 16 for h in halo)
    halo, cells = plan("wide", 0)
    assert halo == [0] * 10 and cells == 10 * 512
    nx, T = 2048, 10
    assert T * (512 + 2 * 1 * nx) > 30000                         # why: one-row halos alone do not fit
    halo, cells = plan("wide", 1)
    assert min(halo) >= 1 and cells == sum((16 + 2 * h) ** 2 for h in halo) <= 30000
    assert plan("t0", 0) == ([], 0)
    halo, cells = plan("slots64", 0)
    assert len(halo) == 6 and min(halo) >= 1
