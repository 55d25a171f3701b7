"""The run-time filter parameters on the HIP map (run with `-m gpu` on an MI355X): the reference's setters and DSPMAP_P_KAPPA / _DETECTION /
_OCCLUSION_MARGIN / _PAIR_CULL_SIGMAS, off the example's values and CHANGED WHILE THE MAP RUNS.

  a  stage parity against the oracle at the points of tests/param_points.py (bars of tests/test_gpu_parity.py)
  b  the schedule of mid-run changes on every way out of the frame -- replayed graph, plain launches with the parameter block by value, plain
     launches with copied parameters, the host-pointer update() -- bit for bit against each other, and a control that skips one change
  c  one frame from the same state against the oracle after a change that arrives AFTER the first frame (frozen birth statics, a captured
     graph that has to go)
  e  a checkpoint written off the defaults, and two slabs under the schedule
(d, the two-branch frame under a table swap, lives with its machinery in tests/test_gpu_round6.py.)

tests/test_runtime_params_cpu.py asserts on the oracle alone that every point and every scheduled change is in effect."""
import numpy as np
import pytest

from tests import common
from tests import param_points as PP
from tests.test_gpu_configs import _slot_exact
from tests.test_gpu_frame_params_by_value import AUTO, CFG, GRAPH, RING, _compare, _Feeder, _frames, _make
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------ a. stage parity off the defaults
@pytest.mark.parametrize("name", [n for n, _ in PP.STAGE_POINTS])
def test_stage_parity_at_parameter_point(dsp, orc, name):
    """bin_points -> predict -> map_update -> add_newborn on oracle and handle from the same injected state with the point's parameters on
    both: observation counts equal; Ck and weights within RTOL (median 1e-6); positions and velocities bit-equal; births slot-exact;
    cursors equal; the newborn normaliser against the oracle's sum of 1 / Ck.  The point differs from the default point on the oracle's own
    output by the bar of test_variant_multiple_neighbors_weight_update, and the two sigmas select the two k_weight instantiations."""
    point = dict(PP.STAGE_POINTS)[name]
    val = PP.point_values(point)
    pts, parts = PP.stage_inputs()
    o = PP.stage_oracle(orc)
    m = dsp.DSPMap(dsp.make_config(**PP.STAGE_CFG))
    m.set_tables(*common.tables(PP.STAGE_SEED))
    n = common.inject_both(o, m, *parts[:5], parts[6])
    assert n > 0.9 * PP.STAGE_PARTICLES
    PP.apply_point_oracle(o, point); PP.apply_point_map(m, dsp.capi, point)
    o.L.dspo_set_current_position(o.h, *PP.STAGE_CUR); m.set_current_position(*PP.STAGE_CUR)
    o.bin_points(pts); m.bin_points(pts)
    o.predict(*PP.STAGE_MOVE); m.predict(*PP.STAGE_MOVE)
    assert m.counters()["n_voxel_full"] == 0  # (overflow winners are order dependent)
    _slot_exact(o, m)
    o.map_update(); m.map_update()
    obs, cnt, ml, lam = m.observations()
    assert np.array_equal(cnt, o.obs_count) and cnt.sum() > 100
    assert lam == pytest.approx(o.L.dspo_expected_newborn(o.h), rel=1e-6)
    nz = np.nonzero(cnt)[0]
    ck_o = np.concatenate([o.obs[b, :cnt[b], 3] for b in nz])
    ck_g = np.concatenate([obs[b, :cnt[b], 3] for b in nz])
    rel = np.abs(ck_g - ck_o) / ck_o
    vo, so, ro, rg = _slot_exact(o, m, cols=(1, 2, 3, 4, 5, 6))
    relw = np.abs(ro[:, 7] - rg[:, 7]) / np.maximum(np.abs(ro[:, 7]), 1e-12)
    print(name, "Ck rel max %.3g median %.3g; weights rel max %.3g median %.3g; variant %s" % (rel.max(), np.median(rel), relw.max(), np.median(relw), m.weight_variant()))
    assert rel.max() < RTOL and np.median(rel) < 1e-6, (rel.max(), np.median(rel))
    assert relw.max() < RTOL and np.median(relw) < 1e-6, (relw.max(), np.median(relw))
    assert m.weight_variant() == ("skip" if val["sigma_ob"] == PP.SIGMA_CULLS else "mask")
    norm_o = float(np.sum(1.0 / ck_o.astype(np.float64)))
    assert m.counters()["newborn_weight"] == pytest.approx(val["nb_weight"] * norm_o, rel=1e-5)
    upd0, born0, slots = PP.oracle_stage_run(PP.DEFAULT_POINT)
    if not PP.is_default(point) and "nb_weight" not in point:
        assert PP.changed_fraction((vo, so, ro), upd0, slots) > PP.IN_EFFECT_FRACTION
    # births: static and dynamic sources, children in the reference's sequential order
    src = PP.stage_birth_sources(orc, pts)
    o.L.dspo_use_velocity_estimator(o.h, 0)
    o.set_birth_cloud(src); m.set_birth_cloud(src)
    o.add_newborn(); m.add_newborn()
    assert o.cursors() == m.cursors()
    vo, so, ro, rg = _slot_exact(o, m, cols=(1, 2, 3, 4, 5, 6))
    nb_o, nb_g = ro[:, 0] > 10, rg[:, 0] > 10
    assert np.array_equal(nb_o, nb_g) and nb_o.sum() == m.counters()["n_born"] > 3000
    relb = np.abs(ro[:, 7] - rg[:, 7]) / np.maximum(np.abs(ro[:, 7]), 1e-12)
    assert relb.max() < RTOL, relb.max()
    assert (ro[nb_o][:, 1] != 0).sum() > 50                                           # dynamic branches exercised
    if "nb_weight" in point and not PP.is_default(point):
        assert PP.changed_fraction((vo[nb_o], so[nb_o], ro[nb_o]), born0, slots) > PP.IN_EFFECT_FRACTION
    o.close(); m.close()


# ------------------------------------------------------------------------------------------------------ b. mid-run changes, path against path
PATHS = (("graph", GRAPH), ("plain_by_value", RING), ("plain_by_size", AUTO), ("plain_copied", 0), ("host_pointer", None))


class _MixedFeeder(_Feeder):
    """_Feeder, with the handles marked host_fed fed through the host-pointer update()"""

    def feed(self, m, f):
        if getattr(m, "host_fed", False):
            pts, pos, quat, t = self.frames[f]
            assert m.update(pts, pos, t, quat) == 1
        else:
            super().feed(m, f)


def _handles(dsp, est, tables, paths=PATHS, seeded=False):
    maps = []
    for name, mode in paths:
        if seeded:   # the handle's own tables, generated from its seed (no injection: DSPMAP_P_REGENERATE_TABLES is live)
            m = dsp.DSPMap(dsp.make_config(seed=4321, table_size=100003, **CFG))
            m.L.dspmap_init_device(m.h)
            if est:
                m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, est)
            if mode is not None:
                m.set_param(dsp.capi.P_USE_GRAPH, mode)
        else:
            m = _make(dsp, est, mode, tables)
        m.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, PP.BASE_CULL_SIGMAS)      # (tests/param_points.py: the switch between 0.03 and 0.1)
        m.host_fed = name == "host_pointer"
        maps.append(m)
    return maps, [name for name, _ in paths]


def _cursors_equal(maps, names, f):
    cur = [m.cursors() for m in maps]
    assert all(c == cur[0] for c in cur), (f, dict(zip(names, cur)))


def _run_schedule(dsp, feeder, maps, names, changes, upto, skip=None, check=True, birth_cloud=False, after=None, start=0):
    """frames start .. upto; the changes of each frame go to every map (but the one named in skip[k]) before a pending clear and the frame;
    all maps equal behind every change and at the end"""
    check_at = {c.frame for c in changes} | {upto}
    for f in range(start, upto + 1):
        todo = PP.at_frame(changes, f)
        for k, m in enumerate(maps):
            for c in todo:
                if not (skip and skip[k] == c.name):
                    c.on_map(m, dsp.capi)
            if PP.clears(f):
                m.clearOccupancyMapPrediction()
            feeder.feed(m, f)
        if check and f in check_at:
            _compare(maps, names, f, birth_cloud)
            _cursors_equal(maps, names, f)
        if after:
            after(f)


def _expected_plain(names, n_frames):
    return [n_frames if n in ("plain_by_value", "plain_by_size") else 0 for n in names]


@pytest.mark.parametrize("est", [0, 2])
def test_schedule_on_every_frame_path(dsp, est, monkeypatch):
    """40 frames, a change every few frames (tests/param_points.py's SCHEDULE: sigma_ob across weight_culls() and back, the pair cull, kappa,
    P_detection, the occlusion margin, newborn weight and number, new tables of other lengths, cursors, and with the estimator its filter
    resolution), a clear of the future accumulators pending before some: handles on DSPMAP_P_USE_GRAPH = 3, 2, 1, 0 fed from the device and
    one fed through update() stay equal in export, results, future status, counters, birth cloud and cursors behind every change and at the
    end.  plain_frames() counts the frames queued as plain launches with the block in the ring: all of them on the handles of values 2
    and 1, none on the graph-forced handle.  It is also 0 on the handle of value 0 (plain launches, copied parameters) and on the host-pointer
    handle, and the library has no counter of graph captures or replays that would tell those two from a replayed graph: that value 0 takes no
    graph is read from dspmap_device_frame (use_graph is false), not asserted here.  The weight update changed its instantiation at the sigma
    changes."""
    import torch
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    frames = _frames(dsp, PP.N_FRAMES, seed=PP.FRAMES_SEED)
    feeder = _MixedFeeder(dsp, torch, frames, False)
    maps, names = _handles(dsp, est, common.tables(5))
    variants = {}

    def after(f):
        variants[f] = [(m.weight_variant(), m.pair_path()) for m in maps]

    _run_schedule(dsp, feeder, maps, names, PP.schedule(est), PP.N_FRAMES - 1, birth_cloud=est == 2, after=after)
    print("weight variant / pair path behind the sigma changes:", variants[2], variants[3], variants[7])
    assert all(v[0] == "mask" for v in variants[2]) and all(v[0] == "skip" for v in variants[3]) and all(v[0] == "mask" for v in variants[7])
    assert variants[3][0][1] == "prepared"                      # (a culling k_weight takes its items from k_pyr_prepare)
    assert [m.plain_frames() for m in maps] == _expected_plain(names, PP.N_FRAMES), [m.plain_frames() for m in maps]
    assert len(maps[0].export_state()[0]) > 1000
    for key, want in ((dsp.capi.P_OBSERVATION_STDDEV, 0.1), (dsp.capi.P_KAPPA, 0.3), (dsp.capi.P_DETECTION, 0.6), (dsp.capi.P_NEWBORN_NUMBER, 32)):
        assert all(m.get_param(key) == pytest.approx(want) for m in maps)
    if est == 2:
        assert maps[1].estimator_path() == "own_stream" and maps[1].estimator_queue()[3] == 0
    for m in maps:
        m.close()


def _differs(a, b):
    sa, sb = a.export_state(), b.export_state()
    return len(sa[0]) != len(sb[0]) or any(not np.array_equal(x, y) for x, y in zip(sa, sb)) or not np.array_equal(a.results(), b.results())


@pytest.mark.parametrize("change", PP.SCHEDULE, ids=lambda c: c.name)
def test_skipped_change_shows_behind_its_frame(dsp, change, monkeypatch):
    """the device-side twin of the oracle-only condition: two graph-forced handles through the schedule up to the frame behind one change,
    which one of them is not given.  They differ there -- a setter that every path ignored alike would pass the path-against-path test and
    fail here -- and were equal in front of it."""
    import torch
    est = 2 if change.estimator_only else 0
    if est == 2:
        monkeypatch.setenv("DSPMAP_XQ_FORCE", "apart")
    frames = _frames(dsp, PP.N_FRAMES, seed=PP.FRAMES_SEED)
    feeder = _MixedFeeder(dsp, torch, frames, False)
    paths = (("graph", GRAPH), ("graph_skips", GRAPH))
    maps, names = _handles(dsp, est, common.tables(5), paths=paths)
    _run_schedule(dsp, feeder, maps, names, PP.schedule(est), change.frame - 1, skip=(None, change.name), check=False)
    assert not _differs(*maps)
    _run_schedule(dsp, feeder, maps, names, PP.schedule(est), change.frame, skip=(None, change.name), check=False, start=change.frame)
    assert _differs(*maps), change
    assert [m.plain_frames() for m in maps] == [0, 0]
    for m in maps:
        m.close()


def test_regenerated_tables_on_every_frame_path(dsp):
    """setPredictionVariance on live handles that generate their own tables (DSPMAP_P_REGENERATE_TABLES after the first frames): the seed is
    set, so every handle regenerates the same tables; all paths stay equal, and a graph-forced handle that keeps its variance differs"""
    import torch
    frames = [fr for fr in _frames(dsp, 30, seed=PP.FRAMES_SEED) if len(fr[0]) >= 255][:12]
    feeder = _MixedFeeder(dsp, torch, frames, False)
    maps, names = _handles(dsp, 0, None, paths=PATHS + (("graph_skips", GRAPH),), seeded=True)
    change = [PP.Change(6, "prediction_variance", "draws", lambda m, c: m.setPredictionVariance(0.12, 0.08), None)]
    skip = (None,) * len(PATHS) + ("prediction_variance",)
    _run_schedule(dsp, feeder, maps, names, change, 5, skip=skip)              # equal, the control too, in front of the change

    def behind(f):   # the paths among themselves, the control apart
        if f in (6, 11):
            _compare(maps[:-1], names[:-1], f, False)
            _cursors_equal(maps[:-1], names[:-1], f)
            assert _differs(maps[0], maps[-1]), f

    _run_schedule(dsp, feeder, maps, names, change, 11, skip=skip, check=False, after=behind, start=6)
    assert [m.plain_frames() for m in maps] == _expected_plain(names, 12)
    assert all(m.get_param(dsp.capi.P_POSITION_STDDEV) == pytest.approx(0.12) for m in maps[:-1])
    for m in maps:
        m.close()


def test_pair_cull_inside_the_zero_radius_is_a_per_pair_rule(dsp):
    """DSPMAP_P_PAIR_CULL_SIGMAS = 4, inside the radius (about 6 sigma) beyond which a term of Ck is zero on its fixed-point grid: what Ck
    adds must still be decided pair by pair, not by which particles share a chunk of k_ck_partial.  A handle that prepares its lists
    (range-sorted chunks) and one whose pair kernels read the lists as the atomics built them (tests/test_gpu_pairs_unsorted.py) chunk
    the same particles differently: obs_ckf, weights, results and counters equal bit for bit.  (Found by the schedule test above, where a
    handle now and then differed from the others in the last bit of a few weights.)"""
    from tests import pair_scenes as S
    from tests.test_gpu_pairs_unsorted import GRAPH as G3, assert_same, frames, handle
    r = S.reference("short_lists")
    sc = r.scene
    a, b = (handle(dsp, sc["cfg"], sc["sigma"], p, G3, cull_sigmas=PP.BASE_CULL_SIGMAS) for p in (1, 2))
    for m in (a, b):
        m.clear_state()
        m.import_state(r.voxel0, r.rec0, r.slot0)
    for f, (sa, sb) in frames([a, b], r.cloud, 3):
        assert (a.pair_path(), b.pair_path()) == ("prepared", "self") and a.weight_variant() == b.weight_variant() == "mask", f
        assert_same(sa, sb, ("cull 4 sigma", f))
    assert sb["counters"]["n_born"] > 1000
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------ c. one frame against the oracle
LATE_CURSORS = (1000, 2000, 300)                     # the cursors both sides start the second frame from, unless the change moves them
SEEDED = dict(seed=4321, table_size=100003)          # a handle that generates its Gaussian tables itself (:1150-1160), from this seed


def _late_change_frame(dsp, orc, path, on_oracle, on_map, estimator=False, seeded=False, min_born=500):
    """One accepted frame on oracle and handle first -- it freezes the birth statics at the example's 20 newborns and, on the graph-forced
    handle, captures the frame --, THEN the change on both, the same state injected into both, one more frame: per-voxel mass within
    RTOL * max(1, |x|) on more than 99.9 % of the voxels, total mass within 1e-4, the position cursor equal (the bars of
    test_single_frame_from_same_state).  estimator: the oracle's restated estimator against the handle's device estimator instead of
    static tags on both sides.  seeded: the handle generates its own Gaussian tables from SEEDED, the oracle gets the same tables from
    dspo_fill_gaussian_tables (the same engine and distribution); the rand() table is injected into both.  -> (oracle, handle, the birth
    clouds of both frames on both sides) for what a case asserts on top."""
    import torch
    pts, parts = PP.stage_inputs()
    o = PP.stage_oracle(orc)
    o.L.dspo_use_velocity_estimator(o.h, 1 if estimator else 2)
    if seeded:
        m = dsp.DSPMap(dsp.make_config(**SEEDED, **PP.STAGE_CFG))
        rtab = common.tables(PP.STAGE_SEED)[2]
        m._chk(m.L.dspmap_set_rand_table(m.h, dsp.capi._ptr(rtab), rtab.size))
        o.set_tables(*filled_tables(orc, 0.05, 0.05, SEEDED["seed"]), rtab)
    else:
        m = dsp.DSPMap(dsp.make_config(**PP.STAGE_CFG))
        m.set_tables(*common.tables(PP.STAGE_SEED))
    m.L.dspmap_init_device(m.h)
    if estimator:
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 2)
    if path == "graph":
        m.set_param(dsp.capi.P_USE_GRAPH, GRAPH)
    dev = torch.from_numpy(pts).cuda()
    pos, q = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)
    clouds = []

    def frame():
        assert o.update(pts, pos, 0.0, q) == 1
        if path == "graph":
            assert m.update_device(dev.data_ptr(), len(pts), pos, 0.0, q) == 1
        else:
            assert m.update(pts, pos, 0.0, q) == 1
        clouds.append((o.get_birth_cloud(), m.get_birth_cloud()))

    frame()
    assert m.counters()["n_born"] > min_born
    o.particles[...] = 0; o.results[...] = 0                  # the oracle's map emptied; inject_both empties the handle's
    n = common.inject_both(o, m, *parts[:5], parts[6])
    assert n > 0.9 * PP.STAGE_PARTICLES
    o.L.dspo_set_cursors(o.h, *LATE_CURSORS); m.set_cursors(*LATE_CURSORS)
    on_oracle(o); on_map(m, dsp.capi)
    frame()                                                   # (same position and stamp: no motion, dt = 0 on both sides)
    assert m.plain_frames() == 0
    occ_o, occ_g = o.results[:, 0], m.results()[:, 0]
    err = np.abs(occ_g - occ_o)
    tol = RTOL * np.maximum(1.0, np.abs(occ_o))
    tot_o, tot_g = occ_o.astype(np.float64).sum(), occ_g.astype(np.float64).sum()
    print(path, "voxels over the bar %d of %d; total mass %.6f / %.6f; born %d" % ((err > tol).sum(), len(err), tot_o, tot_g, m.counters()["n_born"]))
    assert (err <= tol).mean() > 0.999, (err > tol).sum()
    assert abs(tot_g - tot_o) < 1e-4 * tot_o
    assert o.cursors()[0] == m.cursors()[0]
    assert m.counters()["n_born"] > min_born
    return o, m, clouds


def filled_tables(orc, p_stddev, v_stddev, seed, n=SEEDED["table_size"]):
    p, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    orc.lib().dspo_fill_gaussian_tables(p.ctypes.data, v.ctypes.data, n, p_stddev, v_stddev, seed)
    return p, v


@pytest.mark.parametrize("path", ["host_pointer", "graph"])
@pytest.mark.parametrize("change", [c for c in PP.SCHEDULE if c.on_oracle and not c.estimator_only], ids=lambda c: c.name)
def test_single_frame_after_late_change_against_oracle(dsp, orc, change, path):
    """_late_change_frame for every scheduled change the oracle has a counterpart for.  Two scheduled parameters are not here.  The pair
    cull (DSPMAP_P_PAIR_CULL_SIGMAS) is the HIP map's own approximation: the oracle evaluates every pair, so a cull small enough to
    matter has no reference, and one that drops only zeros is test_range_culling_of_pairs_changes_nothing.  The estimator's filter
    resolution needs the estimator on both sides and has the case below, as has setPredictionVariance, which needs generated tables."""
    o, m, _ = _late_change_frame(dsp, orc, path, change.on_oracle, change.on_map)
    o.close(); m.close()


@pytest.mark.parametrize("path", ["host_pointer", "graph"])
def test_single_frame_after_late_filter_resolution_against_oracle(dsp, orc, path):
    """setOriginalVoxelFilterResolution 0.1 -> 0.3 after the first frame, the oracle's restated estimator against the device estimator:
    ground split and cluster tolerance move (:1387-1417), so the second frame's birth cloud is another one than the first frame's -- and
    the same on both sides, point for point, as test_velocity_estimator_matches_oracle_restatement compares --, and the frame holds the
    bars of _late_change_frame."""
    o, m, clouds = _late_change_frame(dsp, orc, path, lambda o: o.L.dspo_set_voxel_filter_resolution(o.h, 0.3),
                                      lambda m, c: m.setOriginalVoxelFilterResolution(0.3), estimator=True)
    key = lambda a: np.lexsort((np.round(a["z"], 4), np.round(a["y"], 4), np.round(a["x"], 4)))
    for w, g in clouds:
        assert len(g) == len(w) > 0
        g, w = g[key(g)], w[key(w)]
        assert np.allclose(g["x"], w["x"]) and np.allclose(g["y"], w["y"]) and np.allclose(g["z"], w["z"])
        assert np.array_equal(g["intensity"] > 0.01, w["intensity"] > 0.01)
        assert np.allclose(g["nx"], w["nx"], atol=1e-3) and np.allclose(g["ny"], w["ny"], atol=1e-3)
    n_dyn = [int((w["intensity"] > 0.01).sum()) for w, _ in clouds]
    assert n_dyn[0] != n_dyn[1] and min(n_dyn) > 10, n_dyn    # the split moved: other points are tagged as clusters behind the change
    assert m.get_param(dsp.capi.P_VOXEL_FILTER_RES) == pytest.approx(0.3)
    o.close(); m.close()


@pytest.mark.parametrize("path", ["host_pointer", "graph"])
def test_single_frame_after_late_prediction_variance_against_oracle(dsp, orc, path):
    """setPredictionVariance(0.12, 0.08) after the first frame on a handle that generates its own tables: DSPMAP_P_REGENERATE_TABLES
    draws both tables again from seed + 1 (:355-360) and leaves the cursors where they are; the oracle is handed the tables
    dspo_fill_gaussian_tables makes from the same seed and deviations.  A handle that kept its first tables would scatter its newborns
    0.05 m wide instead of 0.12 m and miss the per-voxel bar."""
    def on_oracle(o):
        o.L.dspo_set_prediction_variance(o.h, 0.12, 0.08)
        o.set_tables(*filled_tables(orc, 0.12, 0.08, SEEDED["seed"] + 1))
        o.L.dspo_set_cursors(o.h, *LATE_CURSORS)            # (the oracle's set_tables rewinds; the reference's setter and the handle's do not)
    o, m, _ = _late_change_frame(dsp, orc, path, on_oracle, lambda m, c: m.setPredictionVariance(0.12, 0.08), seeded=True)
    assert m.get_param(dsp.capi.P_POSITION_STDDEV) == pytest.approx(0.12)
    o.close(); m.close()


# ------------------------------------------------------------------------------------------------------ e. checkpoint and slabs
def test_checkpoint_off_the_defaults(dsp, tmp_path):
    """a handle that went through the whole schedule is saved; a fresh handle with the example's parameters and ANOTHER pair cull setting
    loads it: get_param returns the saved sigma_ob, kappa, P_detection, newborn weight and number and occlusion margin and the loader's own
    cull setting, and its next two frames equal, bit for bit, those of a twin of the saved handle that is given the loader's cull setting
    (which also holds the frozen static / model split, the two restored fields no getter shows)."""
    import torch
    frames = _frames(dsp, PP.N_FRAMES + 3, seed=PP.FRAMES_SEED)
    feeder = _MixedFeeder(dsp, torch, frames, False)
    paths = (("saved", None), ("twin", None))
    maps, names = _handles(dsp, 0, common.tables(5), paths=paths)
    _run_schedule(dsp, feeder, maps, names, PP.schedule(0), PP.N_FRAMES - 1)
    saved, twin = maps
    path = tmp_path / "off_defaults.ck"
    saved.save_checkpoint(path)
    loader = _make(dsp, 0, None, PP.swap_tables())           # (the tables are the handle's own: the ones the saved handle ended with)
    loader.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, 6.0)
    P = dsp.capi
    assert loader.get_param(P.P_KAPPA) == pytest.approx(0.01) and loader.get_param(P.P_NEWBORN_NUMBER) == 20
    loader.load_checkpoint(path)
    want = {P.P_OBSERVATION_STDDEV: 0.1, P.P_KAPPA: 0.3, P.P_DETECTION: 0.6, P.P_NEWBORN_WEIGHT: 0.002, P.P_NEWBORN_NUMBER: 32, P.P_OCCLUSION_MARGIN: 0.0}
    for key, v in want.items():
        assert loader.get_param(key) == saved.get_param(key) == pytest.approx(v), key
    assert loader.get_param(P.P_PAIR_CULL_SIGMAS) == 6.0 and saved.get_param(P.P_PAIR_CULL_SIGMAS) == 2.0
    assert loader.cursors() == saved.cursors()
    twin.set_param(P.P_PAIR_CULL_SIGMAS, 6.0)
    # (frame 40 of this stream has an empty cloud, so its births would come from the cloud of the last view that had points -- which a
    # checkpoint does not carry, include/dspmap.h: the handles are compared from the first frame with a cloud on)
    assert len(frames[PP.N_FRAMES][0]) == 0 and min(len(frames[PP.N_FRAMES + 1][0]), len(frames[PP.N_FRAMES + 2][0])) >= 255
    for f in (PP.N_FRAMES + 1, PP.N_FRAMES + 2):
        for m in (twin, loader):
            if PP.clears(f):
                m.clearOccupancyMapPrediction()
            feeder.feed(m, f)
        _compare([twin, loader], ["twin", "loader"], f, False)
        _cursors_equal([twin, loader], ["twin", "loader"], f)
    assert twin.counters()["n_live_out"] > 1000 and twin.counters()["n_born"] > 1000
    for m in (saved, twin, loader):
        m.close()


def test_two_slabs_under_the_schedule(dsp):
    """a two-slab group on one GPU (the C++ frame driver) and an unsharded handle on index-order storage, every slab handle and the
    unsharded one given the schedule: the merged slabs equal the unsharded map at the end, slot for slot, as
    test_cpp_driver_group_matches_unsharded compares.  The stream is the one of (b) WITHOUT its empty frames, so a change falls in front of
    another frame than the one tests/test_runtime_params_cpu.py showed it to be in effect for (some in front of a one-point frame): this
    test is about slabs against the unsharded map under the same calls, not about each change showing."""
    import torch
    sharded = __import__("dsp-map_amd.sharded", fromlist=["CppGroup"])
    tables = common.tables(5)
    grp = sharded.CppGroup(dsp, CFG, 2)
    full = dsp.DSPMap(dsp.make_config(**CFG))
    full.set_param(dsp.capi.P_TILING, 0)
    for m in grp.maps + [full]:
        m.set_tables(*tables)
        m.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, PP.BASE_CULL_SIGMAS)
    # (the frames with a cloud, as test_deferred_shares_behind_by_value_frames picks them: the slab driver's tests feed it no empty cloud)
    frames = [fr for fr in _frames(dsp, PP.N_FRAMES + 12, seed=PP.FRAMES_SEED) if len(fr[0]) > 0][:PP.N_FRAMES]
    assert len(frames) == PP.N_FRAMES
    changes = PP.schedule(0)
    moved = 0
    for f, (pts, pos, quat, t) in enumerate(frames):
        for c in PP.at_frame(changes, f):
            for m in grp.maps + [full]:
                c.on_map(m, dsp.capi)
        for m in grp.maps + [full]:
            if PP.clears(f):
                m.clearOccupancyMapPrediction()
        d = torch.from_numpy(pts).cuda()
        assert grp.update(d, pos, t, quat) == 1
        assert full.update_device(d.data_ptr(), len(pts), pos, t, quat) == 1
        grp.sync()
        moved += sum(m.counters()["n_moved"] for m in grp.maps)
    assert full.get_param(dsp.capi.P_TILING) == 0
    got = np.concatenate([m.results() for m in grp.maps], 0)
    assert np.array_equal(got, full.results())
    parts = [m.export_state() for m in grp.maps]
    sv, ss, sr = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.lexsort((ss, sv))
    fv, fs_, fr = full.export_state()
    assert len(fv) > 1000 and moved > 0
    assert np.array_equal(sv[order], fv) and np.array_equal(ss[order], fs_) and np.array_equal(sr[order], fr)
    assert sum(m.counters()["n_live_out"] for m in grp.maps) == full.counters()["n_live_out"]
    assert [m.cursors() for m in grp.maps] == [full.cursors()] * 2
    assert all(m.get_param(dsp.capi.P_NEWBORN_NUMBER) == 32 and m.get_param(dsp.capi.P_KAPPA) == pytest.approx(0.3) for m in grp.maps)
    grp.close(); full.close()
