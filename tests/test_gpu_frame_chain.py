"""The serial frame chain under the product of its switches (run with `-m gpu` on an MI355X)."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("est", [0, 2])
def test_frame_chain_switches_change_nothing(dsp, est):
    """enqueue_frame's serial chain has three switches that only move launches between streams: how the frame is queued
    (DSPMAP_P_USE_GRAPH 0 direct launches + copied parameter block, 1 captured graph, 2 direct launches + parameter ring), where
    the side placement leaves the main chain (DSPMAP_P_SIDE_PLACEMENT 0 behind the list preparation, 1 behind the placement of the
    tiles with a view, 2 behind the prediction) and whether the device estimator's branch shares the side stream.  All nine
    combinations of the first two, placement split forced on (DSPMAP_P_PLACE_SPLIT_TILES = 1), against one single-stream map of
    direct launches, on the map and cloud stream of test_split_placement_changes_nothing (the smallest shape in the suite at which
    both placement launches have tiles): every counter after every frame, and every slot, float and voxel result at the end,
    equal."""
    import torch
    cfg = dict(nx=56, ny=88, nz=12, res=0.15, ppv=24)
    quat = (0.9659258, 0.0, 0.0, 0.258819)   # yawed by 30 degrees
    tables = common.tables(5)
    confs = [(0, None, 2_000_000_000)] + [(g, s * 16 + 3, 1) for g in (0, 1, 2) for s in (0, 1, 2)]
    maps = []
    for graph, side, split in confs:
        m = dsp.DSPMap(dsp.make_config(**cfg)); m.set_tables(*tables)
        m.L.dspmap_init_device(m.h)
        m.set_param(dsp.capi.P_PLACE_SPLIT_TILES, split)
        m.set_param(dsp.capi.P_USE_GRAPH, graph)
        assert m.get_param(dsp.capi.P_USE_GRAPH) == graph
        if side is not None:
            m.set_param(dsp.capi.P_SIDE_PLACEMENT, side)
            assert m.get_param(dsp.capi.P_SIDE_PLACEMENT) == side
        if est:
            m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, est)
        maps.append(m)
    for m in maps:
        m.seed_uniform(2, 0.01, 11, 0.0)
    rng = np.random.default_rng(3)
    ys, zs = np.meshgrid(np.linspace(-2.0, 2.0, 41), np.linspace(-0.9, 0.9, 19))
    base = np.stack([np.full(ys.size, 2.3) + 0.2 * np.sin(2 * ys.ravel()), ys.ravel(), zs.ravel()], 1).astype(np.float32)
    for f in range(6):
        t = f / 30.0
        pts = torch.from_numpy(base + rng.normal(0, 0.004, base.shape).astype(np.float32)).cuda()
        pos = (0.9 * t, 0.5 * t, 0.1 * np.sin(5 * t))
        for m in maps:
            assert m.update_device(pts.data_ptr(), len(base), pos, t, quat) == 1
            m.clearOccupancyMapPrediction()
        ca = maps[0].counters(); ca.pop("update_ms")
        for conf, mb in zip(confs[1:], maps[1:]):
            cb = mb.counters(); cb.pop("update_ms")
            assert ca == cb, (f, conf, ca, cb)
    ref_state, ref_results = maps[0].export_state(), maps[0].results()
    for conf, mb in zip(confs[1:], maps[1:]):
        for a, b in zip(ref_state, mb.export_state()):
            assert np.array_equal(a, b), conf
        assert np.array_equal(ref_results, mb.results()), conf
        got = mb.debug_tile_fov()
        assert 0 < got.sum() < len(got), (conf, got.sum())      # both placement launches had tiles
        if est:   # a split placement keeps the estimator as a forked branch, on the side stream
            assert mb.L.dspmap_debug_estimator_path(mb.h) == 3, conf
    for m in maps:
        m.close()
