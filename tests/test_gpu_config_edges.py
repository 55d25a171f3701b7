"""GPU parity at the edges of the configuration space dspmap_create accepts (tests/config_edges.py; run with `-m gpu`): every stage
against the oracle from scenes that provably touch the edge, every resampling variant the handle may run at the slot edges, whole
frames, captured graph against plain launches, the constructor pre-fill, readout and queries without horizons, state round trips on
full words and ragged cubes, and one map past 2^24 voxels.

The bars are the suite's own: slots and floats of binning, prediction, births and resampling bit-exact, Ck / weights rel 1e-4,
future status rtol 1e-4 / atol 1e-6 and its column totals 2e-6 (_check_resample), counters equal."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import config_edges as E
from tests import query_ref as Q
from tests.test_gpu_parity import RTOL, _birth_sources, gpu_state
from tests.test_gpu_configs import _slot_exact
from tests.test_gpu_round4 import VARIANTS, _check_resample, _force

pytestmark = pytest.mark.gpu

NAMES = list(E.EDGES)
NEWBORNS_PER_POINT = 1
EGO = (0.05, -0.07, 0.0, 0.2)        # a step that makes movers and, into the over-filled box, voxel overflow


def _wg_legal(slots):
    """resample_variant(): four waves per tile up to 48 slots in one word and from 65 to 72 in two"""
    return slots <= 48 or 64 < slots <= 72


def _close(*xs):
    for x in xs:
        x.close()


@pytest.mark.parametrize("name", NAMES)
def test_edge_bin_points(dsp, orc, name):
    o, m = E.make_pair(dsp, orc, name)
    pts = E.observation_cloud(o.cfg)
    q = E.quat_of(name)
    valid = o.bin_points(pts, q)
    m.bin_points(pts, q)
    if E.EDGES[name]["kind"] == "planes":
        E.check_plane_coverage(o)
    obs, cnt, ml, lam = m.observations()
    assert valid > 0 and np.array_equal(cnt, o.obs_count) and np.array_equal(ml, o.obs_max_length)
    oo = o.obs
    for b in np.nonzero(cnt)[0]:
        assert np.array_equal(obs[b, :cnt[b], :3], oo[b, :cnt[b], :3]) and np.array_equal(obs[b, :cnt[b], 4], oo[b, :cnt[b], 4]), b
    assert m.counters()["n_valid"] == valid
    assert lam == pytest.approx(o.L.dspo_expected_newborn(o.h), rel=1e-6)
    _close(o, m)


@pytest.mark.parametrize("name", NAMES)
def test_edge_predict(dsp, orc, name):
    """mapPrediction with movers (up to 3 m/s over 0.2 s: four voxels) and an ego step; arrivals at the full voxels of the over-filled
    box are turned away in the reference's sweep order"""
    kind = E.EDGES[name]["kind"]
    o, m = E.make_pair(dsp, orc, name, seed=3)
    n = E.inject_edge(name, o, m, seed=17, vmax=3.0, newborn_frac=0.0)
    if kind == "slots":
        E.check_slot_coverage(o)
    if kind == "wide":
        E.check_wide_coverage(o)
    pts, q = E.observation_cloud(o.cfg), E.quat_of(name)
    o.bin_points(pts, q); m.bin_points(pts, q)
    o.predict(*EGO); m.predict(*EGO)
    if kind == "slots":
        E.check_slot_coverage(o)
    if kind == "wide":
        E.check_lists_uncut(o)
    vo, so, ro, rg = _slot_exact(o, m)
    c = m.counters()
    assert c["n_live_in"] == n and (c["n_moved"] > 0 or o.V == 1)
    assert c["n_out_of_map"] == n - len(vo) - c["n_voxel_full"] - c["n_pyramid_full"]
    if kind == "slots":
        assert c["n_voxel_full"] > 0
    assert c["n_fov"] == int((o.pyramid_lists[:, :, 0] & 1).sum())
    assert np.array_equal(np.minimum(m.pyramid_counts(), m.capp), (o.pyramid_lists[:, :, 0] != 0).sum(1))
    assert np.array_equal(m.pyramid_candidates(), o.pyramid_candidates)
    _close(o, m)


@pytest.mark.parametrize("name", NAMES)
def test_edge_update_and_birth(dsp, orc, name):
    """mapUpdate and mapAddNewBornParticlesByObservation: Ck and weights to 1e-4, the newborns in the same slots with the same floats"""
    o, m = E.make_pair(dsp, orc, name, seed=61)
    E.inject_edge(name, o, m, seed=23, newborn_frac=0.0)
    pts, q = E.observation_cloud(o.cfg), E.quat_of(name)
    cur = (0.02, -0.01, 0.005)
    o.L.dspo_set_current_position(o.h, *cur); m.set_current_position(*cur)
    o.bin_points(pts, q); m.bin_points(pts, q)
    o.predict(-0.01, 0.0, 0.002, 1 / 30.0); m.predict(-0.01, 0.0, 0.002, 1 / 30.0)
    _slot_exact(o, m)
    o.map_update(); m.map_update()
    obs, cnt, ml, lam = m.observations()
    assert np.array_equal(cnt, o.obs_count) and cnt.sum() > 0
    nz = np.nonzero(cnt)[0]
    ck_o = np.concatenate([o.obs[b, :cnt[b], 3] for b in nz])
    ck_g = np.concatenate([obs[b, :cnt[b], 3] for b in nz])
    rel = np.abs(ck_g - ck_o) / ck_o
    print(name, "Ck rel max", rel.max(), "median", np.median(rel))
    assert rel.max() < RTOL and np.median(rel) < 1e-6, (rel.max(), np.median(rel))
    vo, so, ro, rg = _slot_exact(o, m, cols=(1, 2, 4, 5, 6))
    relw = np.abs(ro[:, 7] - rg[:, 7]) / np.maximum(np.abs(ro[:, 7]), 1e-12)
    print(name, "weight rel max", relw.max())
    assert relw.max() < RTOL, relw.max()
    # births from static and dynamic sources: the sources are the observed points in the map frame (identity attitude: unrotated)
    rng = np.random.default_rng(7)
    view = pts if q[0] == 1.0 else np.stack([-pts[:, 1], pts[:, 0], pts[:, 2]], 1)      # (yaw 90 degrees)
    n_src = min(600, len(view))
    src = _birth_sources(orc, rng, view[:n_src], cur, n_dyn=min(60, n_src // 2))
    o.L.dspo_use_velocity_estimator(o.h, 0)
    o.set_birth_cloud(src); m.set_birth_cloud(src)
    o.add_newborn(); m.add_newborn()
    assert o.cursors() == m.cursors()
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    nb_o, nb_g = ro[:, 0] > 10, rg[:, 0] > 10
    assert nb_o.sum() == nb_g.sum() == m.counters()["n_born"] > 0
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    assert np.array_equal(vo[ko], vg[kg]) and np.array_equal(so[ko], sg[kg])
    assert np.array_equal(ro[ko][:, 1:7], rg[kg][:, 1:7])
    assert np.array_equal(ro[ko][:, 0] > 10, rg[kg][:, 0] > 10)
    assert np.allclose(ro[ko][:, 7], rg[kg][:, 7], rtol=RTOL)
    if E.EDGES[name]["kind"] == "slots":
        born = so[nb_o]
        assert born.max() == o.slots - 1 and (o.slots <= 64 or (born >= 64).any())      # newborns up to the last slot
    _close(o, m)


def _resample_cases():
    out = []
    for name in NAMES:
        if name == "wide":
            out += [(name, v, -1) for v in ("wg+windows", "wave+windows")]
        elif name in E.TWO_WORD or name == "slots64":
            out += [(name, v, sp) for v in VARIANTS for sp in (0, 1)]
        else:
            out.append((name, None, -1))
    return out


@pytest.mark.parametrize("name,variant,sparse", _resample_cases())
def test_edge_resample(dsp, orc, name, variant, sparse):
    """mapOccupancyCalculationAndResample; at the slot edges under every variant the handle may run -- {four waves per tile, one wave}
    x {rollout inline / light, k_rollout windows} x {dense, sparse instantiation} -- checked to have run; where the map is outside what
    the four-wave resampler was built for (49 - 64 and 73 - 128 slots) the handle must have refused it"""
    kind = E.EDGES[name]["kind"]
    o, m = E.make_pair(dsp, orc, name, seed=5)
    T = o.T
    if variant is not None:
        want = _force(m, dsp, variant)
        if sparse >= 0:
            m.set_param(dsp.capi.P_SPARSE_SWEEP, sparse)
        if not _wg_legal(o.slots):
            want = 0 | ((1 if VARIANTS[variant][1] else 2) << 1)          # refused: one wave per tile, k_rollout light / windows
    E.inject_edge(name, o, m)
    before = E.check_slot_coverage(o) if kind == "slots" else None
    o.occupancy_resample(); m.occupancy_resample()
    var, n_win, n_dir = m.rollout_paths()
    if variant is not None:
        assert var == want, (var, want)
        assert (var & 1) == (1 if variant.startswith("wg") and _wg_legal(o.slots) else 0)
    if T == 0:
        assert var >> 1 == 3
    if kind == "slots":
        E.check_slot_coverage(o, need_full=False)
        E.check_resample_coverage(o, before)
    if kind == "wide":
        assert m.rollout_plan()[0] == [0] * T and var >> 1 == 2 and n_win > 0, (var, n_win, n_dir)     # the collapsed plan ran
    if T > 0:
        fut = _check_resample(o, m, T)
    else:
        res_g, res_o = m.results(), o.results
        assert np.array_equal(res_g[:, 0], res_o[:, 0]) and np.array_equal(res_g[:, 1:3], res_o[:, 1:3])
        vo, so, ro, rg = _slot_exact(o, m, cols=(1, 2, 4, 5, 6))
        assert np.allclose(ro[:, 7], rg[:, 7], rtol=1e-6) and m.counters()["n_live_out"] == len(vo)
    partner = E.EDGES[name].get("partner")
    if partner is not None:                                                # the other storage order: the same bits
        o2, m2 = E.make_pair(dsp, orc, name, seed=5, tiling=partner)
        E.inject_edge(name, o2, m2)
        m2.occupancy_resample()
        if kind == "wide":
            assert min(m2.rollout_plan()[0]) >= 1
        assert np.array_equal(m2.getFutureStatus(), fut) and np.array_equal(m2.results(), m.results())
        for a, b in zip(gpu_state(m), gpu_state(m2)):
            assert np.array_equal(a, b)
        _close(o2, m2)
    _close(o, m)


@pytest.mark.parametrize("name", NAMES)
def test_edge_whole_frames_and_graph(dsp, orc, name):
    """three update() frames from the injected state against dspo_update (the bars of test_e_shaped_whole_frames), then the captured
    graph against plain launches: bit-identical.
    Every fourth point of the cloud and ONE newborn per point instead of the example's twenty: on these 2.4 m maps twenty put 16 and
    more equal-weight newborns into an empty voxel, and thinning n equal weights to M = 12 puts resampling thresholds (j + 1/2) n / M on
    exact ties.  The frame's newborn weight is one ulp from the oracle's for some clouds (a known residue) and flips
    them: measured on t0 and t16 alike, 3 voxels chose another survivor in frame 0 (weights 0.51627475 against 0.5162747) and, the
    newborn weight being normalised over the whole -- here tiny -- map, 62 to 132 of 1536 voxels were past 1e-4 in frame 1.  With at
    most M newborns per voxel nothing is thinned on a tie; that drift is not what an edge case is about."""
    o, m = E.make_pair(dsp, orc, name, seed=71)
    E.inject_edge(name, o, m, seed=31, newborn_frac=0.0)
    pts, q = E.observation_cloud(o.cfg)[::4], E.quat_of(name)
    o.L.dspo_use_velocity_estimator(o.h, 2)
    o.L.dspo_set_newborn_number(o.h, NEWBORNS_PER_POINT); m.setNewBornParticleNumberofEachPoint(NEWBORNS_PER_POINT)
    for f in range(3):
        pos = (0.01 * f, 0.0, 0.004 * f)
        assert o.update(pts, pos, f / 30.0, q) == 1
        assert m.update(pts, pos, f / 30.0, q) == 1
        occ_o, occ_g = o.results[:, 0], m.results()[:, 0]
        err = np.abs(occ_g - occ_o)
        tol = RTOL * np.maximum(1.0, np.abs(occ_o))
        print(name, "frame", f, "voxels past tol", int((err > tol).sum()), "of", o.V)
        assert (err <= tol).mean() > (0.999 if f == 0 else 0.99), (f, (err > tol).sum())
        assert abs(occ_g.astype(np.float64).sum() - occ_o.astype(np.float64).sum()) < (1e-4 if f == 0 else 2e-3) * occ_o.sum()
        if f == 0:
            assert o.cursors()[0] == m.cursors()[0]
        xo, fo = o.get_occupancy_with_future(0.2)
        ng, xg, fg = m.getOccupancyMapWithFutureStatus(0.2)
        assert np.allclose(fg.sum(0), fo.sum(0), rtol=5e-3)
    _close(o, m)
    runs = []
    for graph in (1, 0):
        o2, m2 = E.make_pair(dsp, orc, name, seed=71)
        m2.set_param(dsp.capi.P_USE_GRAPH, graph)
        m2.setNewBornParticleNumberofEachPoint(NEWBORNS_PER_POINT)
        E.inject_edge(name, o2, m2, seed=31, newborn_frac=0.0)
        for f in range(3):
            assert m2.update(pts, (0.01 * f, 0.0, 0.004 * f), f / 30.0, q) == 1
        runs.append(gpu_state(m2) + (m2.results(), m2.getFutureStatus()))
        _close(o2, m2)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert len(runs[0][0]) > 0


@pytest.mark.parametrize("name", ["slots64", "slots66", "slots128", "m1"])
def test_edge_constructor_prefill(dsp, orc, name):
    """addRandomParticles (:594-624) with as many particles as the map has slots: about half of the voxels fill to the last slot and
    turn the rest away, in the reference's sequential order"""
    o, m = E.make_pair(dsp, orc, name)
    n = o.V * o.slots
    o.L.dspo_add_random_particles(o.h, n, 0.01)
    m._chk(m.L.dspmap_add_random_particles(m.h, n, 0.01))
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    per_voxel = np.bincount(vo, minlength=o.V)
    assert (per_voxel == o.slots).any() and (per_voxel < o.slots).any() and so.max() == o.slots - 1
    assert len(vo) == len(vg)
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    assert np.array_equal(vo[ko], vg[kg]) and np.array_equal(so[ko], sg[kg]) and np.array_equal(ro[ko], rg[kg])
    assert set(np.unique(rg[:, 0]).tolist()) == {15.0}
    assert o.cursors() == m.cursors()
    _close(o, m)


def test_edge_t0_readout_and_queries(dsp, orc):
    """no prediction horizons: the readouts write no future status (and do not crash), a query at t >= 0 reads the current mass"""
    o, m = E.make_pair(dsp, orc, "t0")
    E.inject_edge("t0", o, m)
    o.occupancy_resample(); m.occupancy_resample()
    assert m.rollout_paths()[0] >> 1 == 3
    guard = np.full(64, 7.0, np.float32)
    m._chk(m.L.dspmap_get_future(m.h, guard.ctypes.data_as(C.c_void_p)))
    xyz = np.zeros((m.V, 3), np.float32)
    n = C.c_int()
    m._chk(m.L.dspmap_get_occupancy_with_future(m.h, 0.2, xyz.ctypes.data_as(C.c_void_p), m.V, C.byref(n), guard.ctypes.data_as(C.c_void_p)))
    assert (guard == 7.0).all()
    n_o = o.L.dspo_get_occupancy_map(o.h, 0.2, None, 0)
    assert n.value == n_o > 0 and m.getFutureStatus().shape == (m.V, 0)
    rng = np.random.default_rng(3)
    half = common.half_extent(o.cfg)
    smp = np.concatenate([rng.uniform(-1.1, 1.1, (4000, 3)) * np.array(half), rng.choice([-1.0, 0.0, 0.3, 5.0], (4000, 1))], 1).astype(np.float32)
    res = m.results()
    for radius in (0.0, 0.2):
        want, flags = Q.query(o.cfg, res, np.zeros((m.V, 0), np.float32), smp, radius=radius)
        got = m.query_occupancy(smp, radius=radius)
        assert np.array_equal(got, want)
    inside = ~Q.query(o.cfg, res, np.zeros((m.V, 0), np.float32), smp)[1]
    assert np.array_equal(m.query_occupancy(smp)[inside], res[Q.own_voxel(o.cfg, smp[:, :3])[1][inside], 0])      # the current mass, whatever t
    _close(o, m)


@pytest.mark.parametrize("name", ["slots128", "ragged_cubes"])
def test_edge_state_round_trip(dsp, orc, name, tmp_path):
    """export_state -> clear_state -> import_state -> export_state is the identity; a checkpoint saved on cubes loads into an
    index-order handle with the same records"""
    o, m = E.make_pair(dsp, orc, name, tiling=1)
    n = E.inject_edge(name, o, m)
    v0, s0, r0 = gpu_state(m)
    assert len(v0) == n and s0.max() == m.slots - 1
    vo, so, ro = o.export_sparse()
    ko = np.lexsort((so, vo))
    assert np.array_equal(v0, vo[ko]) and np.array_equal(s0, so[ko]) and np.array_equal(r0[:, 1:], ro[ko][:, 1:])
    m.clear_state()
    assert len(gpu_state(m)[0]) == 0
    m.import_state(v0, r0, s0)
    for a, b in zip((v0, s0, r0), gpu_state(m)):
        assert np.array_equal(a, b)
    path = tmp_path / "edge.ck"
    m.save_checkpoint(path)
    m2 = dsp.DSPMap(dsp.make_config(**E.EDGES[name]["cfg"]))
    m2.set_param(dsp.capi.P_TILING, 0)
    m2.load_checkpoint(path)
    for a, b in zip((v0, s0, r0), gpu_state(m2)):
        assert np.array_equal(a, b)
    _close(o, m, m2)


def test_zz_map_past_two_to_the_24_voxels(dsp, orc):
    """512 x 512 x 68 at two particles per voxel (17.8 M voxels, 71 M cells): a sparse state with particles in the highest-numbered
    voxels, movers across the top layers, the constructor pre-fill, resampling and the result grid, slot-exact against the oracle.
    (Named to run last in the file: the largest map.)"""
    o = orc.Oracle(orc.make_config(**E.BIG))
    m = dsp.DSPMap(dsp.make_config(**E.BIG))
    p, v, r = common.tables(9, nrand=600011)
    o.set_tables(p, v, r); m.set_tables(p, v, r)
    assert o.V == m.V > 1 << 24
    half = common.half_extent(o.cfg)
    rng = np.random.default_rng(4)
    n = 400000
    px, py, pz, vx, vy, w = common.random_particles(41, n, half, vmax=2.0, static_frac=0.3, wlo=0.002, whi=0.05)
    pz[: n // 2] = rng.uniform(half[2] - 0.6, half[2] * 0.999, n // 2).astype(np.float32)       # the four top layers: voxels past 2^24
    placed = common.inject_both(o, m, px, py, pz, vx, vy, w)
    vo = o.export_sparse()[0]
    assert placed > 0.95 * n and (vo >= 1 << 24).sum() > 0.4 * n and vo.max() > o.V - 512 * 512
    q = (1.0, 0.0, 0.0, 0.0)
    empty = np.zeros((0, 3), np.float32)
    o.bin_points(empty, q); m.bin_points(empty, q)
    o.predict(0.05, -0.07, 0.0, 0.2); m.predict(0.05, -0.07, 0.0, 0.2)
    vo, so, ro, rg = _slot_exact(o, m)
    c = m.counters()
    assert c["n_live_in"] == placed and c["n_moved"] > 0.3 * placed
    assert c["n_out_of_map"] == placed - len(vo) - c["n_voxel_full"] - c["n_pyramid_full"]
    # the pre-fill on top: its particles land everywhere, the top layers included
    k = 600000
    o.L.dspo_add_random_particles(o.h, k, 0.01)
    m._chk(m.L.dspmap_add_random_particles(m.h, k, 0.01))
    vo, so, ro = o.export_sparse()
    vg, sg, rg = gpu_state(m)
    assert ((ro[:, 0] > 10) & (vo >= 1 << 24)).sum() > 1000
    ko, kg = np.lexsort((so, vo)), np.lexsort((sg, vg))
    assert len(vo) == len(vg) and np.array_equal(vo[ko], vg[kg]) and np.array_equal(so[ko], sg[kg])
    assert np.array_equal(ro[ko][:, 0] > 10, rg[kg][:, 0] > 10)          # (the oracle's old particles carry its in-view flag 7)
    for col in range(1, 8):
        bad = np.nonzero(ro[ko][:, col] != rg[kg][:, col])[0]
        assert len(bad) == 0, (col, len(bad), vo[ko][bad[:4]], ro[ko][bad[:4]], rg[kg][bad[:4]])
    assert o.cursors() == m.cursors()
    o.occupancy_resample(); m.occupancy_resample()
    _check_resample(o, m, 1)
    assert (o.results[1 << 24:, 0] > 0).sum() > 1000
    _close(o, m)
