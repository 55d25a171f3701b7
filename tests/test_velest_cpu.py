"""What the scenes of tests/velest_scenes.py claim about themselves, pinned with the oracle on the CPU: these are conditions on the
INPUTS of tests/test_gpu_velest_scale.py, so that no GPU test can pass by missing the path it was built for."""
import numpy as np
import pytest

from tests import velest_scenes as vs

F = np.float32
SCENES = list(vs.BUILDERS)


def analyse(orc, pts, outside):
    """view -> world -> ground split -> clusters (the oracle's), sizes, fp32 centroids in ascending index order, static test"""
    view = pts[pts[:, 0] > 0] if outside else pts
    w = vs.world(view)
    ng = w[w[:, 2] > vs.RES_F]
    label, K = orc.euclidean_clusters(ng, float(vs.TOL))
    sizes = np.bincount(label[label >= 0], minlength=K)
    feat = np.zeros((K, 4), F)
    for c in range(K):
        m = ng[label == c]
        acc = np.cumsum(m, axis=0, dtype=F)[-1]          # sequential fp32 sums, the reference's order
        feat[c, :3] = acc / F(len(m))
        feat[c, 3] = len(m)
    dyn = (sizes <= 200) & (feat[:, 2] <= F(1.5))
    return dict(n_view=len(view), ng=ng, label=label, K=K, sizes=sizes, feat=feat, dyn=dyn, dropped=int((label < 0).sum()))


@pytest.fixture(scope="module")
def analysed(orc):
    cache = {}

    def get(name):
        if name not in cache:
            sc = vs.scene(name)
            cache[name] = [analyse(orc, p, sc.expect["outside"][f] > 0) for f, p in enumerate(sc.frames)]
        return cache[name]
    return get


@pytest.mark.parametrize("name", SCENES)
def test_scene_is_in_view_and_in_range(orc, name):
    sc = vs.scene(name)
    o = orc.Oracle(orc.make_config(**vs.CFG))
    for f, pts in enumerate(sc.frames):
        assert pts.dtype == F and pts.shape[1] == 3
        assert o.bin_points(pts, sc.quat) == len(pts) - sc.expect["outside"][f], f      # the oracle's field-of-view test
        seen = pts[pts[:, 0] > 0]
        assert len(seen) == len(pts) - sc.expect["outside"][f]
        if sc.expect["in_map"]:
            assert np.abs(seen[:, :2]).max() < 4.95 and np.abs(seen[:, 2]).max() < 3.0
        else:
            assert seen[:, 0].max() < 7.6
        assert len(pts) <= 6144                                                           # what the device estimator takes
    o.close()
    # deterministic: a second build gives the same bits
    again = vs.BUILDERS[name]()
    assert all(np.array_equal(a, b) for a, b in zip(again.frames, sc.frames))


@pytest.mark.parametrize("name", SCENES)
def test_cluster_counts_sizes_and_birth_cloud(orc, analysed, name):
    sc = vs.scene(name)
    ex = sc.expect
    run = vs.oracle_run(orc, name)
    for f, a in enumerate(analysed(name)):
        assert a["K"] == ex["K"][f], (f, a["K"])
        assert ex["sizes"] <= set(a["sizes"].tolist()), (f, sorted(ex["sizes"] - set(a["sizes"].tolist())))
        assert a["sizes"].min() >= 5
        assert int(a["dyn"].sum()) == ex["n_dyn"][f], (f, int(a["dyn"].sum()))
        assert np.abs(a["feat"][:, 2] - 1.5).min() > 1e-3                      # no static test hangs on the last bits of a centroid
        assert a["dropped"] == ex["dropped"][f], (f, a["dropped"])
        birth = run[f]["birth"]
        assert len(birth) == a["n_view"] - a["dropped"], f
        assert int((birth["intensity"] > 0.01).sum()) == int(a["sizes"][a["dyn"]].sum()), f
        # many equal sizes: the order of the clusters is decided by their seeds
        assert len(set(a["sizes"].tolist())) < a["K"] // 2
    if "min_K" in ex:
        assert ex["K"][0] >= ex["min_K"]


@pytest.mark.parametrize("name", SCENES)
def test_matching_sizes_and_step_counts(orc, analysed, name):
    """max(n_dyn, n_last) of every frame and the number of passes through the do-while body of the oracle's Hungarian on that frame's
    cost matrix; the restatement that counts them gives the oracle's assignment"""
    sc = vs.scene(name)
    ex = sc.expect
    frames = analysed(name)
    for f in range(1, len(frames)):
        cur, last = frames[f]["feat"][frames[f]["dyn"]], frames[f - 1]["feat"][frames[f - 1]["dyn"]]
        if ex["hungarian"][f] is not None:
            assert (len(cur), len(last)) == ex["hungarian"][f], f
        cost, gate = vs.cost_matrix(cur, last)
        assign, steps = vs.hungarian_steps(cost)
        assert np.array_equal(assign, orc.hungarian(cost)), f
        N = max(cost.shape)
        T = N * (N + 1) // 2
        claim = ex["steps"][f]
        print(name, "frame", f, "nr x nc", cost.shape, "steps", steps, "gated", float(1 - gate.mean()))
        if claim == "T":
            assert steps == T and not gate.any(), (f, steps, T)
        elif claim == "<=2N":
            assert N <= steps <= 2 * N, (f, steps, N)
        else:
            assert N <= steps <= T, (f, steps, N, T)
            assert gate.any() and not gate.all()                                 # gated and real-valued costs side by side


def test_hungarian_edge_sizes():
    nd = vs.HUNGARIAN_EDGE_NDYN
    pairs = {(nd[f], nd[f - 1]) for f in range(1, len(nd))}
    assert {(64, 64), (65, 64), (64, 65), (65, 65), (130, 70), (70, 130)} <= pairs


@pytest.mark.parametrize("K", [63, 64, 65, 128, 129])
def test_k_edge_special_clusters(orc, analysed, K):
    name = "k_edge_%d" % K
    sc = vs.scene(name)
    frames = analysed(name)
    run = vs.oracle_run(orc, name)
    for f, a in enumerate(frames):
        cz = a["feat"][:, 2]
        assert ((cz > 1.5) & (cz < 1.51)).sum() == 1 and ((cz > 1.49) & (cz <= 1.5)).sum() == 1, f
        assert (a["sizes"] == 201).sum() == 1 and not a["dyn"][a["sizes"] == 201].any()
        # the big clusters' members are spread over the slices of k_ve_components
        big = np.nonzero(a["label"] == 0)[0]
        per = -(-len(a["ng"]) // 32)
        assert len(set((big // per).tolist())) >= 24, f
        # ground: the two neighbouring sums around res_filter
        w = vs.world(sc.frames[f])
        z_lo, z_hi = vs._ground_straddle()
        lo_w, hi_w = F(z_lo + F(1.0)), F(z_hi + F(1.0))
        assert lo_w <= vs.RES_F < hi_w and np.nextafter(z_lo, F(0)) == z_hi
        assert (w[:, 2] == lo_w).sum() == sc.expect["ground_points"] - sc.expect["ground_above"]
        assert (w[:, 2] == hi_w).sum() == sc.expect["ground_above"] and (w[:, 2] <= vs.RES_F).sum() == (w[:, 2] == lo_w).sum()
        # the chain: consecutive points at d2 == tol2 in fp32 (no fused multiply-add), every other pair farther
        ch = vs.world(sc.expect["chains"][f])
        assert np.array_equal(ch, sc.expect["chains"][f] + np.array(vs.POS))       # exactly representable
        d2 = vs.d2_f32(ch[:, None, :], ch[None, :, :])
        n = len(ch)
        for i in range(n):
            for j in range(i + 1, n):
                assert (d2[i, j] == vs.TOL2) if j == i + 1 else (d2[i, j] > vs.TOL2), (i, j, d2[i, j])
        assert orc.euclidean_clusters(ch, float(vs.TOL))[1] == 1
        assert orc.euclidean_clusters(ch, float(np.nextafter(vs.TOL, F(0))), min_size=1)[1] == n
    # frame 1: every cluster moves 0.03 .. 0.3 m, but for the one that is faster than 5 m/s
    b1 = run[1]["birth"]
    dynp = b1["intensity"] > 0.01
    zeroed = dynp & (b1["nx"] == 0) & (b1["ny"] == 0) & (b1["nz"] == 0)
    assert (zeroed & (np.abs(b1["x"] - 3.9) < 1e-3)).sum() == 12                # the 12-point stick at 6.2 m/s: matched, zeroed
    # 20 -> 130 points: a pair that only the size gate closes (the assignment then pairs the grown cluster with a neighbour's
    # predecessor about 1 m away -- the minimum-cost assignment, faster than 5 m/s and zeroed as well)
    c0, c1 = frames[0]["feat"][frames[0]["dyn"]], frames[1]["feat"][frames[1]["dyn"]]
    dist = np.sqrt(((c1[:, None, :3].astype(np.float64) - c0[None, :, :3]) ** 2).sum(-1))
    dn = np.abs(c1[:, None, 3] - c0[None, :, 3])
    assert ((dn > 100) & (dist < 0.3)).sum() == 1
    moving = dynp & (b1["nx"] > -100) & ~zeroed
    assert moving.sum() > 0.8 * dynp.sum()                                        # the others found their predecessors
    speed = np.sqrt(b1["nx"].astype(np.float64) ** 2 + b1["ny"] ** 2 + b1["nz"] ** 2)[moving]
    assert 0.29 <= speed.min() and speed.max() <= 3.0, (speed.min(), speed.max())   # 0.03 .. 0.3 m in 0.1 s
    # frame 2: a third of the clusters are gone and as many stand where nothing stood (the survivors moved < 0.1 m)
    c2 = frames[2]["feat"][frames[2]["dyn"]]
    dist = np.sqrt(((c2[:, None, :3].astype(np.float64) - c1[None, :, :3]) ** 2).sum(-1))
    assert (dist.min(1) > 0.2).sum() >= K // 3 and (dist.min(0) > 0.2).sum() >= K // 3


def test_all_gated_has_no_match(orc):
    b = vs.oracle_run(orc, "all_gated_128")[1]["birth"]
    assert len(b) == len(vs.scene("all_gated_128").frames[1]) and (b["intensity"] > 0.01).all() and (b["nx"] == F(-10000)).all()


def test_dense_cells_and_snakes(orc, analysed):
    sc = vs.scene("dense")
    ex = sc.expect
    tol = vs.TOL
    for f, a in enumerate(analysed("dense")):
        assert len(sc.frames[f]) == ex["n_points"] == 6144 and a["n_view"] == 6144 - 400
        cells = np.floor((a["ng"] / tol).astype(F)).astype(np.int64)            # the kernel's cell of a point
        assert len(np.unique(cells, axis=0)) >= ex["min_cells"], len(np.unique(cells, axis=0))
        assert ((a["sizes"] >= 150) & (a["sizes"] <= 200)).sum() == 4
    # the outside points are scattered through the input order
    where = np.nonzero(sc.frames[0][:, 0] <= 0)[0]
    assert len(where) == 400 and where.min() < 100 and where.max() > 6000 and np.diff(where).max() < 200
    # a snake is one cluster through its bridges alone: below the tolerance it falls into its runs and the bridge points
    for p, segs in ex["snakes"]:
        w = vs.world(p)
        assert np.array_equal(w, p + np.array(vs.POS))
        assert orc.euclidean_clusters(w, float(tol))[1] == 1
        label, n = orc.euclidean_clusters(w, float(np.nextafter(tol, F(0))), min_size=1)
        assert n == 2 * segs - 1


def test_rand_wrap_wraps():
    sc = vs.scene("rand_wrap")
    assert sc.r_cursor == vs.NRAND - 20 and sc.r_cursor + sc.expect["K"][0] > vs.NRAND
    assert all(np.array_equal(a, b) for a, b in zip(sc.frames, vs.scene("k_edge_65").frames))
