"""GPU tests of the SELF-MAPPED pair kernels (k_ck_partial_self, k_weight<false, true>; DSPMAP_P_PAIR_PREPARE): whole frames whose pair
kernels map their work items themselves and read the pyramid lists as they were registered -- no k_pyr_prepare launch -- against the same
frames on an identical handle that prepares its lists (DSPMAP_P_PAIR_PREPARE = 1), BIT FOR BIT: every particle record (the weights among
them), obs_ckf, the results grid, the occupancy words (voxel / slot of every live particle), the counters and the item counts.  part_inv
has no accessor of its own: the counter newborn_weight is w_nb times its sum, reduced in a fixed order.

Which path ran is read back (DSPMap.pair_path), not assumed.  Every coverage condition is computed from the ORACLE's state on the CPU.

  * the dense scenes of tests/pair_scenes.py: the two "mask" scenes take the self-mapped kernels (both chunk sizes), `culled` and `wide5x5`
    (k_weight<true>) must report that they stayed on the prepared path;
  * a 32x32x12 map with 6 degree pyramids (np = 112, not 448; capp = 438) whose list lengths sit on the chunk edges: P = 0, 1, 31, 32, 33, 63, 64, 65,
    255, 256, 257, pyramids nobody observes (O = 0: no Ck item, one weight item), O = 64 | 65 and 128 | 129 (wu_split), and the same
    lists under 5x5 neighbourhoods;
  * overfull lists (the maps of tests/test_gpu_list_capacity.py: lists past CAPA, spill-pool entries, turned-away stayers, re-slotted
    arrivals): the sort, the cut and k_place_fix's pass inside the Ck launch, against the prepared path and the oracle, and the handle's
    fall-back to the prepared path (DSPMAP_P_PAIR_PREPARE = 0) until its state is cleared;
  * captured and plain-launch frames, and the parameter flipped in mid-run.
"""
import functools
import types

import numpy as np
import pytest

from tests import common
from tests import pair_scenes as S

pytestmark = pytest.mark.gpu

QUAT = (1.0, 0.0, 0.0, 0.0)
GRAPH, PLAIN = 3, 2          # DSPMAP_P_USE_GRAPH: the frame as one captured graph / as plain launches


# ------------------------------------------------------------------------------------------------------------------ helpers
def snapshot(m):
    """everything the pair kernels' work shows up in after a whole frame (syncs)"""
    c = m.counters()
    c.pop("update_ms")
    obs, cnt, maxlen, lam = m.observations()
    return dict(state=m.export_state(), ckf=obs[:, :, 3].copy(), obs_cnt=cnt.copy(), lam=lam, results=m.results().copy(), counters=c,
                items=m.pair_items(), lists=m.pyramid_counts().copy(), cand=m.pyramid_candidates().copy())


def assert_same(a, b, what):
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(x, y), what                          # voxel, slot (the occupancy words), records: weights bit for bit
    for k in ("ckf", "obs_cnt", "results", "lists", "cand"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["lam"] == b["lam"] and a["items"] == b["items"], (what, a["items"], b["items"])
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def handle(dsp, cfg, sigma, prepare, graph, tables_seed=1, cull_sigmas=None):
    m = dsp.DSPMap(dsp.make_config(**cfg))
    m.set_tables(*common.tables(tables_seed))
    m.setObservationStdDev(sigma)
    if cull_sigmas is not None:
        m.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, cull_sigmas)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 0)                  # every point in view a static birth source: the frame is device-resident
    m.set_param(dsp.capi.P_USE_GRAPH, graph)
    m.set_param(dsp.capi.P_PAIR_PREPARE, prepare)
    assert m.get_param(dsp.capi.P_PAIR_PREPARE) == prepare
    return m


def frames(maps, cloud, n, start=0, each=None):
    """n identical frames on every map; yields (frame, [snapshot per map]) after each"""
    import torch
    d = torch.from_numpy(np.array(cloud, np.float32)).cuda()          # (a copy: the scenes are read-only)
    for f in range(start, start + n):
        for m in maps:
            if each:
                each(f, m)
            assert m.update_device(d.data_ptr(), len(cloud), (0.0, 0.0, 0.0), f / 30.0, QUAT) == 1
        yield f, [snapshot(m) for m in maps]


# ------------------------------------------------------------------------------------------------------------------ dense scenes
@pytest.mark.parametrize("graph", [GRAPH, PLAIN])
@pytest.mark.parametrize("name", ["short_lists", "long_lists"])
def test_self_mapped_frames_equal_prepared_frames_dense(dsp, orc, name, graph):
    r = S.reference(name)
    S.check_scene(r)
    sc = r.scene
    a, b = (handle(dsp, sc["cfg"], sc["sigma"], p, graph) for p in (1, 2))
    for m in (a, b):
        m.clear_state()
        m.import_state(r.voxel0, r.rec0, r.slot0)
    for f, (sa, sb) in frames([a, b], r.cloud, 3):
        assert (a.pair_path(), b.pair_path()) == ("prepared", "self"), f
        assert a.weight_variant() == b.weight_variant() == "mask"
        assert_same(sa, sb, (name, f))
        if f == 0:                                                 # the lists of the oracle's prediction: nothing moves, nothing born yet
            assert np.array_equal(sb["lists"], r.P) and np.array_equal(sb["obs_cnt"], r.obs_count)
            assert sb["items"] == S.expected_items(r)
            assert (sb["ckf"] != 0).sum() == r.obs_count.sum()
    assert sb["counters"]["n_born"] > 1000
    a.close(); b.close()


@pytest.mark.parametrize("name", ["culled", "wide5x5"])
def test_maps_that_branch_over_far_pairs_stay_prepared(dsp, orc, name):
    r = S.reference(name)
    sc = r.scene
    m = handle(dsp, sc["cfg"], sc["sigma"], 2, GRAPH)
    m.clear_state()
    m.import_state(r.voxel0, r.rec0, r.slot0)
    for f, (s,) in frames([m], r.cloud, 1):
        assert m.weight_variant() == "skip" and m.pair_path() == "prepared"
        assert s["items"] == S.expected_items(r)
    m.close()


# ------------------------------------------------------------------------------------------------------------------ chunk edges
EDGE_CFG = dict(nx=32, ny=32, nz=12, res=0.15, ppv=24, angle=6)
EDGE_P = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
EDGE_NPH, EDGE_NPV = 14, 8
# observations per pyramid, per column h (equal on all rows): three empty columns (O = 0 in columns 0 and 1), then sums of 63 and 126 ...
EDGE_COLUMNS = (0, 0, 0, 2, 6, 7, 7, 7, 14, 14, 14, 14, 14, 14)
# ... which these bins raise to exactly 64, 65, 128, 129 around (column, row)
EDGE_EXACT = {(6, 2): 64, (6, 5): 65, (10, 2): 128, (10, 5): 129}
# the pyramids whose lists are cut to EDGE_P: columns 4 .. 9 of the two middle rows (the longest pyramids of the map), all observed
EDGE_AT = [(h, v) for v in (3, 4) for h in range(4, 10)][:len(EDGE_P)]
PER_VOXEL = 22


def edge_counts():
    cnt = np.repeat(np.asarray(EDGE_COLUMNS, np.int64)[:, None], EDGE_NPV, axis=1)
    for (h, v), target in EDGE_EXACT.items():
        cnt[h, v] += target - cnt[h - 1:h + 2, v - 1:v + 2].sum()
    return cnt


@functools.lru_cache(maxsize=None)
def edge_reference(neighbor_n):
    """the oracle's state of the chunk-edge scene (once per process, copied out): particles per pyramid cut to EDGE_P in EDGE_AT, a fan of
    observations with edge_counts() points per pyramid"""
    from oracle import oracle_py as orc
    cfg = dict(EDGE_CFG, neighbor_n=neighbor_n) if neighbor_n else dict(EDGE_CFG)
    o = orc.Oracle(orc.make_config(**cfg))
    o.set_tables(*common.tables(1))
    o.L.dspo_set_observation_stddev(o.h, 0.1)
    npv = o.cfg.half_fov_v * 2 // o.cfg.angle_resolution
    assert npv == EDGE_NPV and o.NP == EDGE_NPH * EDGE_NPV != 448
    o.bin_points(np.zeros((0, 3), np.float32))                      # (the planes of the identity attitude)
    rng = np.random.default_rng(5)
    # observations: random directions inside the field of view, 0.8 .. 2.0 m, the first cnt[h, v] of every pyramid
    pool = 40000
    az, el = np.radians(rng.uniform(-41.9, 41.9, pool)), np.radians(rng.uniform(-23.9, 23.9, pool))
    dirs = np.stack([np.ones(pool), np.tan(az), np.tan(el)], 1)
    pts = (rng.uniform(0.8, 2.0, pool)[:, None] * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    bp = S._pyramid_of(o, pts)
    cnt = edge_counts()
    take = [np.nonzero(bp == b)[0][:cnt.ravel()[b]] for b in range(o.NP)]
    assert all(len(t) == c for t, c in zip(take, cnt.ravel()))
    cloud = pts[rng.permutation(np.concatenate(take))]
    # particles: PER_VOXEL in every voxel, static; the lists of EDGE_AT cut to EDGE_P
    px, py, pz, vx, vy, w = common.uniform_per_voxel(o.cfg, PER_VOXEL, 9)
    b = S._pyramid_of(o, np.stack([px, py, pz], 1))
    keep = np.ones(len(px), bool)
    want = {h * npv + v: target for (h, v), target in zip(EDGE_AT, EDGE_P)}
    for q in range(o.NP):                                           # (the other lists: 40 .. 400 entries, below this map's capp of 438)
        idx = np.nonzero(b == q)[0]
        target = want.get(q, int(rng.integers(40, 401)))
        assert len(idx) >= target or q not in want, (q, len(idx), target)
        keep[idx[target:]] = False
    px, py, pz, vx, vy, w = (a[keep] for a in (px, py, pz, vx, vy, w))
    o.inject(px, py, pz, vx, vy, np.zeros_like(px), w, 1.0)
    r = types.SimpleNamespace(cfg=cfg, cloud=cloud, cnt_table=cnt, capp=o.capp, NP=o.NP)
    r.voxel0, r.slot0, r.rec0 = o.export_sparse()
    assert len(r.voxel0) == len(px)                                 # nobody was dropped by a full voxel
    r.n_valid = o.bin_points(cloud)
    o.predict(0.0, 0.0, 0.0, 1 / 30.0)
    r.obs_count = o.obs_count.copy()
    nbs = (2 * max(1, neighbor_n) + 1) ** 2 + 1
    r.lists, r.cand = o.pyramid_lists.copy(), o.pyramid_candidates.copy()
    r.nb = o._view(o.L.dspo_neighbor_table(o.h), (o.NP, nbs), np.int32).copy()
    r.P = (r.lists[:, :, 0] & 1).sum(1)
    r.O = np.array([r.obs_count[r.nb[q, 1:1 + r.nb[q, 0]]].sum() for q in range(o.NP)])
    o.close()
    return r


def check_edges(r, neighbor_n):
    """what the chunk-edge scene must reach (oracle state only)"""
    assert r.n_valid == len(r.cloud) == r.cnt_table.sum()
    assert np.array_equal(r.obs_count.reshape(r.cnt_table.shape), r.cnt_table)
    assert r.cand.max() <= r.capp and np.array_equal(r.cand, r.P)                   # no list is cut
    for (h, v), target in zip(EDGE_AT, EDGE_P):
        assert r.P[h * EDGE_NPV + v] == target, (h, v)
        assert r.O[h * EDGE_NPV + v] > 0                                            # P = 0 with observations: chunk 0's duties alone
    assert r.P.sum() <= S.CK_SMALL_FOV                                              # items of 32 particles: the edges above are chunk edges
    assert ((r.O == 0) & (r.P > 0)).sum() >= 8                                      # no Ck item, one weight item or more
    assert ((r.P > S.WU_TPB) & (r.O > 0)).sum() >= 2
    if neighbor_n < 2:
        for x in (64, 65, 128, 129):
            assert ((r.O == x) & (r.P > 0)).sum() >= 1, x
    else:
        assert r.nb[:, 0].max() == 25 and r.O.max() > 256                           # full 5x5 neighbourhoods, eight lanes per particle


@pytest.mark.parametrize("graph", [GRAPH, PLAIN])
@pytest.mark.parametrize("neighbor_n", [0, 2])
def test_self_mapped_frames_at_the_chunk_edges(dsp, orc, neighbor_n, graph):
    r = edge_reference(neighbor_n)
    check_edges(r, neighbor_n)
    a, b = (handle(dsp, r.cfg, 0.1, p, graph) for p in (1, 2))
    for m in (a, b):
        m.clear_state()
        m.import_state(r.voxel0, r.rec0, r.slot0)
    for f, (sa, sb) in frames([a, b], r.cloud, 3):
        assert (a.pair_path(), b.pair_path()) == ("prepared", "self"), f
        assert b.weight_variant() == "mask"
        assert_same(sa, sb, (neighbor_n, f))
        if f == 0:
            assert np.array_equal(sb["lists"], r.P) and np.array_equal(sb["obs_cnt"], r.obs_count)
            assert sb["items"] == S.expected_items(r)
    a.close(); b.close()


def test_parameter_flipped_in_mid_run(dsp, orc):
    """1 -> 2 -> 0 -> 2 on one handle (a captured frame per path: the path is part of the graph's key), against a handle that stays at 1"""
    r = edge_reference(0)
    a, b = handle(dsp, r.cfg, 0.1, 1, GRAPH), handle(dsp, r.cfg, 0.1, 1, GRAPH)
    for m in (a, b):
        m.clear_state()
        m.import_state(r.voxel0, r.rec0, r.slot0)
    seq = [1, 1, 2, 2, 0, 0, 2, 1]
    paths = []

    def flip(f, m):
        if m is b:
            m.set_param(dsp.capi.P_PAIR_PREPARE, seq[f])

    for f, (sa, sb) in frames([a, b], r.cloud, len(seq), each=flip):
        paths.append(b.pair_path())
        assert a.pair_path() == "prepared"
        assert_same(sa, sb, f)
    assert paths == ["prepared" if p == 1 else "self" for p in seq], paths
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ overfull lists
FULL_MAP = dict(nx=160, ny=40, nz=16, res=0.15, ppv=24, angle=3)


def _full_pair(dsp, orc, prepares, graph, vmax):
    """the oracle and one HIP handle per entry of `prepares`, from the same state whose pyramid lists are far past CAPA (the whole-frame
    map of tests/test_gpu_list_capacity.py); the HIP handles evaluate every pair (k_weight<false>: the self-mapped kernels are legal)"""
    o = orc.Oracle(orc.make_config(**FULL_MAP))
    o.set_tables(*common.tables(3))
    px, py, pz, vx, vy, w = common.uniform_per_voxel(o.cfg, 12, 7, vmax=vmax)
    o.inject(px, py, pz, vx, vy, np.zeros_like(px), w, 1.0)
    state = o.export_sparse()
    maps = []
    for p in prepares:
        m = _full_handle(dsp, p, graph)
        m.clear_state()
        m.import_state(state[0], state[2], state[1])
        maps.append(m)
    return o, maps, state


def _full_handle(dsp, prepare, graph):
    m = dsp.DSPMap(dsp.make_config(**FULL_MAP))
    m.set_tables(*common.tables(3))
    m.set_param(dsp.capi.P_PAIR_CULL_SIGMAS, 1e6)
    m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, 0)
    m.set_param(dsp.capi.P_USE_GRAPH, graph)
    m.set_param(dsp.capi.P_PAIR_PREPARE, prepare)
    return m


@pytest.mark.parametrize("graph", [GRAPH, PLAIN])
def test_overfull_lists_inside_the_ck_launch(dsp, orc, graph):
    """lists far past CAPA, every particle moving: the self-mapped Ck launch sorts, cuts and re-slots (= 2) exactly as k_pyr_prepare and
    k_place_fix's riders do (= 1) -- bit for bit -- and as the oracle does: the first frame's removals are the oracle's, the occupancy
    within the bars of test_whole_frames_past_list_capacity_against_oracle.  A handle left at 0 falls back to the prepared path after the
    first such frame and returns to the self-mapped kernels when its state is cleared."""
    import torch
    from tests.test_gpu_parity import RTOL
    o, (a, b, z), state = _full_pair(dsp, orc, (1, 2, 0), graph, vmax=1.5)
    o.L.dspo_use_velocity_estimator(o.h, 2)                     # (the oracle's static tags: every point in view a zero-velocity birth source)
    pts = common.wall_cloud(7, n_side=48, dist=7.0, half_w=2.6, half_h=1.0)
    d = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    reslotted = 0
    for f in range(3):
        pos, t = (0.02 * f, -0.01 * f, 0.0), f / 30.0
        for m in (a, b, z):
            assert m.update_device(d.data_ptr(), len(pts), pos, t, QUAT) == 1
        sa, sb, sz = (snapshot(m) for m in (a, b, z))
        assert (a.pair_path(), b.pair_path()) == ("prepared", "self") and b.weight_variant() == "mask"
        assert z.pair_path() == ("self" if f == 0 else "prepared"), f               # the sticky fall-back
        assert_same(sa, sb, f)
        assert_same(sa, sz, f)
        c = sb["counters"]
        assert c["n_overflow_inexact"] == 0, c
        reslotted += c["n_reslotted"]
        if f == 0:
            assert o.update(pts, pos, t, QUAT) == 1
            past = int((sb["cand"] > common.capa(b.capp)).sum())
            assert past >= 20, past                                                 # lists past CAPA: spill-pool entries
            assert np.array_equal(o.pyramid_candidates, sb["cand"])
            removed_o = int(np.maximum(o.pyramid_candidates - o.capp, 0).sum())
            assert removed_o > 100000 and c["n_pyramid_full"] == removed_o, (c["n_pyramid_full"], removed_o)
            occ_o, occ_g = o.results[:, 0], sb["results"][:, 0]
            err = np.abs(occ_g - occ_o)
            tol = RTOL * np.maximum(1.0, np.abs(occ_o))
            assert (err <= tol).mean() > 0.999, (err > tol).sum()
            assert abs(occ_g.astype(np.float64).sum() - occ_o.astype(np.float64).sum()) < 1e-4 * occ_o.sum()
        else:
            assert c["n_pyramid_full"] > 0                                          # later frames cut again
    # a turned-away particle handed its slot to an arrival behind it: k_place_fix's pass moved one (the oracle's sweep does this whenever a
    # full list turns a particle away in a voxel that arrivals enter after it: removed_o > 0 with every particle moving)
    assert reslotted > 0
    # cleared (and restored): the handle is back on the self-mapped kernels
    z.clear_state()
    z.import_state(state[0], state[2], state[1])
    assert z.update_device(d.data_ptr(), len(pts), (0.0, 0.0, 0.0), 1.0, QUAT) == 1
    z.sync()
    assert z.pair_path() == "self"
    assert z.update_device(d.data_ptr(), len(pts), (0.0, 0.0, 0.0), 1.0 + 1 / 30.0, QUAT) == 1
    assert z.pair_path() == "prepared"
    o.close()
    for m in (a, b, z):
        m.close()
