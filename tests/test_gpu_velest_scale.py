"""The device velocity estimator (dspmap_velest.hip) past its small-scene paths, bit for bit against the oracle: 63 / 64 / 65 clusters
(one radix pass or two), 128 / 129 (cluster records in LDS or in global memory), matchings of 64 / 65 / 130 rows or columns (cost
matrix in LDS or in the global scratch matrix; rectangular both ways), an all-gated matching, a 6 144-point cloud with more occupied
cells than hash buckets, and a rand() cursor that wraps.  The scenes and what they guarantee: tests/velest_scenes.py, pinned on the CPU
by tests/test_velest_cpu.py.  Nothing here is compared with a tolerance: the centroid sums run in the reference's order and the matching
is in double precision on both sides."""
import numpy as np
import pytest

from tests import common
from tests import velest_scenes as vs

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "z", "nx", "ny", "nz", "intensity")


def _handle(dsp, sc, queue, newborn=vs.NEWBORN):
    m = dsp.DSPMap(dsp.make_config(**vs.CFG))
    m.set_tables(*common.tables(1))
    if newborn is not None:
        m.set_param(dsp.capi.P_NEWBORN_NUMBER, newborn)     # (see velest_scenes.oracle_run: the cursors then follow from the birth cloud)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    if queue is not None:
        m.set_param(dsp.capi.P_ESTIMATOR_QUEUE, queue)
    if sc.r_cursor is not None:
        m.set_cursors(0, 0, sc.r_cursor)
    return m


def _same_birth_cloud(m, ref, f):
    g, w = m.get_birth_cloud(), ref["birth"]
    assert len(g) == len(w), (f, len(g), len(w))
    for k in FIELDS:
        assert np.array_equal(g[k], w[k]), (f, k, int((g[k] != w[k]).sum()))
    assert m.cursors()[0] == ref["cursors"][0] and m.cursors()[2] == ref["cursors"][2], (f, m.cursors(), ref["cursors"])


@pytest.mark.parametrize("name", list(vs.BUILDERS))
def test_device_estimator_equals_oracle(dsp, orc, name):
    """per frame: the same points in the same order, bit-equal velocities, the intensities inherited through the matches, the position
    and rand() cursors -- with the estimator as a forked branch of the frame (no cross-queue wait that could give up)"""
    sc = vs.scene(name)
    ref = vs.oracle_run(orc, name)
    m = _handle(dsp, sc, queue=0)
    for f, pts in enumerate(sc.frames):
        assert m.update(pts, sc.pos, sc.stamp(f), sc.quat) == 1
        assert m.L.dspmap_debug_estimator_path(m.h) == 3, f
        _same_birth_cloud(m, ref[f], f)
        m.getOccupancyMapWithFutureStatus(0.2)
    m.close()


def test_device_resident_frame_equals_host_buffer_frame(dsp):
    """k_edge(129) through update_device on a second handle ends in the same map as through the host-buffer call"""
    import torch
    sc = vs.scene("k_edge_129")
    a, b = _handle(dsp, sc, queue=0, newborn=None), _handle(dsp, sc, queue=0, newborn=None)
    for f, pts in enumerate(sc.frames):
        dev = torch.from_numpy(pts).cuda()
        assert a.update(pts, sc.pos, sc.stamp(f), sc.quat) == 1
        assert b.update_device(dev.data_ptr(), len(pts), sc.pos, sc.stamp(f), sc.quat) == 1
        assert b.L.dspmap_debug_estimator_path(b.h) == 3, f
        a.getOccupancyMapWithFutureStatus(0.2); b.getOccupancyMapWithFutureStatus(0.2)
    sa, sb = a.export_state(), b.export_state()
    assert len(sa[0]) > 1000
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    a.close(); b.close()


K_Q = 128


@pytest.mark.parametrize("name", ["all_gated_%d" % K_Q, "k_edge_129"])
def test_estimator_on_its_own_queue_keeps_up(dsp, orc, name):
    """the default DSPMAP_P_ESTIMATOR_QUEUE: the frame's first birth kernel waits at most 200 ms for the estimator, then runs without
    its birth stage and the NEXT call fails.  K_Q = 128 is the largest measured size whose worst case (an all-gated matching:
    8 256 steps) stays below half of that wait: 16.8 ms on the frame's critical path (tools/velest_scaling.py; 300 clusters: 127 ms).
    No wait gives up, the call after the last frame succeeds, and the birth clouds are the oracle's."""
    import torch
    sc = vs.scene(name)
    ref = vs.oracle_run(orc, name)
    m = _handle(dsp, sc, queue=None)
    assert m.get_param(dsp.capi.P_ESTIMATOR_QUEUE) == 1
    clouds = [torch.from_numpy(p).cuda() for p in sc.frames]
    for f, pts in enumerate(sc.frames):
        assert m.update_device(clouds[f].data_ptr(), len(pts), sc.pos, sc.stamp(f), sc.quat) == 1, f
        assert m.L.dspmap_debug_estimator_path(m.h) in (1, 2), f     # 2: the streams share a hardware queue, the forked fallback
        _same_birth_cloud(m, ref[f], f)
        m.getOccupancyMapWithFutureStatus(0.2)
    n = len(sc.frames)
    assert m.update_device(clouds[0].data_ptr(), len(sc.frames[0]), sc.pos, sc.stamp(n), sc.quat) == 1      # no give-up error
    m.sync()
    assert m.estimator_queue()[3] == 0
    m.close()
