"""GPU test of the binding's torch call paths (dsp-map_amd/capi.py): for every wrapper with a device branch, the result for a CUDA tensor
equals the result for the same numbers as numpy byte for byte -- dicts, tuples and tensors compared field by field against the
structured dtype the host route returns.  One 16 x 16 x 6 map at 0.15 m after five frames of the wall cloud, every layer built once.

Per wrapper: n = 0, 1 and 65 inputs (one full wave plus one lane), each as a contiguous tensor and as a non-contiguous view (so that the
binding's .contiguous() makes a temporary); the handle once on torch's current stream and once on a side stream (dspmap_set_stream), the
input produced by a kernel on torch's stream immediately before the call and the output consumed on torch's stream immediately after,
with no synchronisation in between.  A call the library refuses (an empty input, where it refuses one) has to be refused with the same
text on both routes; n = 65 has to succeed.  The zero-copy device lists equal their host copies."""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu
F = np.float32
SHAPE, RES = (16, 16, 6), 0.15
S2 = float(np.sqrt(0.5))
QUATS = [(1.0, 0.0, 0.0, 0.0), (S2, 0.0, 0.0, S2), (0.9799247, 0.0868241, 0.1736482, 0.0)]
NS = [0, 1, 65]
N_FIELDS, MAX_STEPS, MAX_LEN = 2, 40, 24


class Env:
    pass


@pytest.fixture(scope="module", params=["current", "side"])
def env(request, dsp):
    """the map, its layers, torch's stream for the test and where the handle queues: on that stream or on another one"""
    e = Env()
    e.dsp, e.mode = dsp, request.param
    e.torch_stream = torch.cuda.Stream()
    e.handle_stream = e.torch_stream if request.param == "current" else torch.cuda.Stream()
    m = e.m = dsp.DSPMap(dsp.make_config(nx=SHAPE[0], ny=SHAPE[1], nz=SHAPE[2], res=RES, ppv=12, seed=7))
    m._chk(m.L.dspmap_init_device(m.h))
    m._chk(m.L.dspmap_set_stream(m.h, e.handle_stream.cuda_stream))
    pts = (common.wall_cloud(3, n_side=40) * F(0.6 / 3.0)).astype(F)
    e.cur = np.array([0.05, -0.03, 0.0], F)
    for f in range(5):
        assert m.update(pts, e.cur, f / 30.0, QUATS[f % 3]) == 1
        m.integrate_known()
    mass = m.results()[:, 0]
    e.thr = float(np.median(mass[mass > 0]))
    m.build_distance_field(e.thr, 6)
    m.build_cast_grid(e.thr, 0)
    m.build_forecast([0.0, 0.4, 1.1])
    m.build_frontiers(-1.0, 10, 1, 4)
    m.build_objects(-1.0, 26, 1, 4096)
    m.update_tracks(0.1)
    grid = m.cast_grid()
    bits = np.unpackbits(grid.view(np.uint8), axis=-1, bitorder="little")[..., :SHAPE[0]].astype(bool)   # [L, nz, ny, nx]
    e.free = np.argwhere(~bits.any(0))                                                                    # (z, y, x), free in every layer
    assert len(e.free) >= 65 and bits.any(), "the scene leaves too little free or nothing occupied"
    e.half = np.array(common.half_extent(m.cfg), np.float64)
    yield e
    m.close()


def _samples(e, n, width, seed):
    """[n, width] float32: positions over and a little beyond the map; the time columns (3, and 7 of a segment) -1, inside a horizon, past
    the last one; a view's quaternion, range and time"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, width), F)
    a[:, 0:3] = rng.uniform(-1.1, 1.1, (n, 3)) * e.half
    if width == 4:
        a[:, 3] = rng.choice(np.array([-1.0, 0.3, 1.0, 5.0], F), n)
    elif width == 8:
        a[:, 4:7] = a[:, 0:3] + rng.uniform(-0.8, 0.8, (n, 3))
        a[:, 3] = rng.choice(np.array([-1.0, 0.0, 0.3], F), n)
        a[:, 7] = a[:, 3] + rng.choice(np.array([0.0, 0.5, 2.5], F), n)
    else:
        a[:, 0:3] = rng.uniform(-0.9, 0.9, (n, 3)) * e.half
        quat = rng.standard_normal((n, 4))
        a[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        a[:, 7] = rng.uniform(0.5, 3.0, n)
        a[:, 8] = rng.choice(np.array([-1.0, 0.3], F), n)
    return a


def _points(e, n, seed, free=False):
    """REACH_POINT_DTYPE [n], field k % N_FIELDS: anywhere over the map, or the centres of cells that are free in every layer"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, e.dsp.capi.REACH_POINT_DTYPE)
    if free:
        c = e.free[rng.choice(len(e.free), n, replace=False)]
        xyz = (c[:, ::-1] + 0.5) * float(F(RES)) - e.half
    else:
        xyz = rng.uniform(-1.05, 1.05, (n, 3)) * e.half
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["field"] = np.arange(n) % N_FIELDS
    return p


def _dev(a, contiguous):
    """the numbers of a as a CUDA tensor that a kernel on torch's current stream has just written (a structured array as its float32 rows):
    contiguous, or a view of every other column / entry of a wider tensor"""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(F).reshape(len(a), a.dtype.itemsize // 4)
    t = torch.from_numpy(a).cuda()
    if contiguous:
        return t.clone()
    v = torch.stack([t, t], -1)[..., 0]       # element stride 2: not contiguous for any n >= 1, a single row included
    assert t.numel() <= 1 or not v.is_contiguous()
    return v


def _outcome(e, fn):
    try:
        return fn()
    except e.dsp.capi.DSPMapError as err:
        return "DSPMapError: %s" % err


def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = (x + 0).cpu().numpy()          # consumed by a kernel on torch's stream first, no synchronisation before it
    return np.ascontiguousarray(x).tobytes()


def _same(host, dev, tag):
    """a device result against the host result of the same numbers"""
    if isinstance(host, str) or isinstance(dev, str):
        assert host == dev, tag
    elif isinstance(host, tuple):
        assert isinstance(dev, tuple) and len(dev) == len(host), tag
        for k, (h, d) in enumerate(zip(host, dev)):
            _same(h, d, tag + (k,))
    elif isinstance(dev, np.ndarray):      # (what a build left behind, read through the host getter after either route)
        assert dev.dtype == host.dtype and dev.shape == host.shape and _bytes(dev) == _bytes(host), tag
    elif isinstance(dev, dict):
        assert list(dev) == list(host.dtype.names), tag
        for k in dev:
            want = torch.float32 if host.dtype[k].base == F else torch.int32
            assert dev[k].dtype == want and tuple(dev[k].shape) == host[k].shape, tag + (k,)
            assert _bytes(dev[k]) == _bytes(host[k]), tag + (k,)
    else:
        assert isinstance(dev, torch.Tensor) and dev.is_cuda, tag
        if host.dtype.names:
            assert dev.dtype == torch.int32 and tuple(dev.shape) == host.shape + (host.dtype.itemsize // 4,), tag
        else:
            assert dev.dtype == (torch.float32 if host.dtype == F else torch.int32) and tuple(dev.shape) == host.shape, tag
        assert _bytes(dev) == _bytes(host), tag


def _both(e, n, tag, call, *inputs):
    """call(*inputs) with numpy inputs, then with each tensor form of them; n = 65 must not be refused; returns the host result"""
    with torch.cuda.stream(e.torch_stream):
        host = _outcome(e, lambda: call(*inputs))
        assert n < 65 or not isinstance(host, str), (tag, host)
        for contiguous in (True, False):
            dev = _outcome(e, lambda: call(*[_dev(a, contiguous) for a in inputs]))
            _same(host, dev, (e.mode, tag, n, contiguous))
    return host


@pytest.mark.parametrize("n", NS)
def test_queries(env, n):
    m, q = env.m, _samples(env, n, 4, 1)
    occ = _both(env, n, "query_occupancy", lambda a: m.query_occupancy(a, radius=0.2, outside=0.5), q)
    _both(env, n, "query_occupancy world", lambda a: m.query_occupancy(a, world=True), q)
    traj = _samples(env, n * 3, 4, 2).reshape(n, 3, 4)
    _both(env, n, "trajectory_risk", lambda a: m.trajectory_risk(a, radius=0.2, threshold=env.thr), traj)
    dist = _both(env, n, "query_distance", lambda a: m.query_distance(a, outside=9.0), q)
    _both(env, n, "query_distance grad=False", lambda a: m.query_distance(a, grad=False), q)
    _both(env, n, "query_forecast", lambda a: m.query_forecast(a), q)
    _both(env, n, "query_forecast lerp", lambda a: m.query_forecast(a, lerp=True, world=True), q)
    known = _both(env, n, "query_known", lambda a: m.query_known(a), q)
    _both(env, n, "query_objects", lambda a: m.query_objects(a), q)
    if n == 65:
        assert (occ > 0).any() and (occ == 0.5).any() and (dist[0] > 0).any() and (dist[1] != 0).any() and (known >= 0).any()


@pytest.mark.parametrize("n", NS)
def test_casts_and_boxes(env, n):
    m, s = env.m, _samples(env, n, 8, 3)
    hits = _both(env, n, "cast_segments", lambda a: m.cast_segments(a), s)
    _both(env, n, "cast_segments world", lambda a: m.cast_segments(a, world=True), s)
    boxes = _both(env, n, "grow_boxes", lambda a: m.grow_boxes(a, (4, 4, 2)), s)
    _both(env, n, "grow_boxes with_current", lambda a: m.grow_boxes(a, (1, 2, 3), with_current=True), s)
    if n == 65:
        assert len(set(hits["status"].tolist())) >= 2 and (boxes["status"] == env.dsp.capi.BOX_OK).any()


@pytest.mark.parametrize("n", NS)
def test_views(env, n):
    m, v = env.m, _samples(env, n, 9, 4)
    sc = _both(env, n, "score_views", lambda a: m.score_views(a, 2), v)
    sets = _samples(env, n * 2, 9, 5).reshape(n, 2, 9)
    _both(env, n, "score_view_sets", lambda a: m.score_view_sets(a, 2), sets)
    _both(env, n, "score_view_sets scores", lambda a: m.score_view_sets(a, 2, scores=True), sets)
    _both(env, n, "select_views", lambda a: m.select_views(a, min(3, n), 2), v)
    _both(env, n, "select_views scores", lambda a: m.select_views(a, min(3, n), 2, n_fixed=min(1, n), scores=True), v)
    if n == 65:
        assert (sc["n_seen"] > 0).any()


@pytest.mark.parametrize("n", NS)
def test_reach_builds_and_paths(env, n):
    m = env.m
    src, starts = _points(env, n, 6, free=True), _points(env, n, 7)
    kw = dict(t_start=0.0, step_seconds=0.05, max_steps=MAX_STEPS)
    still = dict(t_start=-1.0, step_seconds=0.0, max_steps=MAX_STEPS)      # (reach_paths descends time-invariant fields only)
    fields = _both(env, n, "build_reach_fields", lambda a: (m.build_reach_fields(a, N_FIELDS, **still), m.reach_field(None, N_FIELDS))[1], src)
    if n == 0 and isinstance(fields, str):
        m.build_reach_fields(_points(env, 4, 6, free=True), N_FIELDS, **still)
    _both(env, n, "reach_paths", lambda a: m.reach_paths(a, MAX_LEN), starts)
    _both(env, n, "reach_paths max_len=0", lambda a: m.reach_paths(a, 0, world=True), starts)
    sets = _both(env, n, "build_reach_timeline", lambda a: (m.build_reach_timeline(a, N_FIELDS, **kw), m.reach_sets(1))[1], src)
    if n == 0 and isinstance(sets, str):
        m.build_reach_timeline(_points(env, 4, 6, free=True), N_FIELDS, **kw)
    steps, cells = _both(env, n, "reach_timeline_paths", lambda a: m.reach_timeline_paths(a, MAX_LEN), starts)
    _both(env, n, "reach_timeline_paths max_len=0", lambda a: m.reach_timeline_paths(a, 0), starts)
    if n == 65:
        assert (fields < env.dsp.capi.REACH_UNREACHED).any() and sets.shape[0] == MAX_STEPS + 1 and (steps > 0).any() and (cells >= 0).any()


@pytest.mark.parametrize("n", NS)
def test_cost_builds_paths_and_shortening(env, n):
    m = env.m
    src, starts = _points(env, n, 8, free=True), _points(env, n, 9)
    build = lambda a: (m.build_cost_fields(a, N_FIELDS, bands=[(0.3, 2)], max_cost=200), m.cost_field(None, N_FIELDS))[1]   # noqa: E731
    fields = _both(env, n, "build_cost_fields", build, src)
    if n == 0 and isinstance(fields, str):
        build(_points(env, 4, 8, free=True))
    cost, cells = _both(env, n, "cost_paths", lambda a: m.cost_paths(a, MAX_LEN), starts)
    _both(env, n, "cost_paths max_len=0", lambda a: m.cost_paths(a, 0), starts)
    for max_seg in (None, 0, 3):
        _both(env, n, "shorten_paths max_seg=%s" % max_seg, lambda s, c: m.shorten_paths(s, c, window=8, max_seg=max_seg), cost, cells)
    info = _both(env, n, "shorten_paths timed", lambda s, c: m.shorten_paths(s, c, t_start=0.0, step_seconds=0.05), cost, cells)[0]
    if n == 65:
        assert (fields < env.dsp.capi.COST_UNREACHED).any() and (cost > 0).any() and (info["n_segments"] > 0).any()


def test_device_lists_equal_their_host_copies(env):
    m, capi = env.m, env.dsp.capi
    with torch.cuda.stream(env.torch_stream):
        n_cells, n_blocks, _ = m.frontier_counts()
        n_objects = m.object_counts()[0]
        print(env.mode, "frontier cells", n_cells, "blocks", n_blocks, "objects", n_objects, "tracks", m.track_counts()[0])
        assert n_cells > 0 and n_blocks > 0 and n_objects > 0
        for name, dtype in (("frontier_cells", None), ("frontier_blocks", capi.FRONTIER_BLOCK_DTYPE), ("objects", capi.OBJECT_DTYPE),
                            ("object_labels", None), ("tracks", capi.TRACK_DTYPE)):
            host = getattr(m, name)()
            dev = getattr(m, name)(device="cuda")
            assert host.dtype == (dtype or np.int32) and len(host) > 0, name
            _same(host, dev, (env.mode, name))


def test_device_route_shape_errors_keep_their_texts(env):
    """what a CUDA tensor of the wrong dtype or shape raises, text for text (the host route's texts are in tests/test_capi_calls_cpu.py);
    nothing is enqueued"""
    m = env.m

    def t(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    samples = "%s: a float32 tensor of shape [..., %d]"
    points = "%s: a float32 / int32 tensor of shape [n, 4] holding dspmap_reach_point rows"
    cases = [(lambda: m.query_occupancy(t(5, 3)), samples % ("query_occupancy", 4)), (lambda: m.query_distance(t(5, 4, dtype=torch.float64)), samples % ("query_distance", 4)),
             (lambda: m.query_forecast(t(5, 5)), samples % ("query_forecast", 4)), (lambda: m.query_known(t(5, 4, dtype=torch.int32)), samples % ("query_known", 4)),
             (lambda: m.query_objects(t(4)[:3]), samples % ("query_objects", 4)), (lambda: m.trajectory_risk(t(5, 3, 3)), samples % ("trajectory_risk", 4)),
             (lambda: m.trajectory_risk(t(5, 4)), "trajectory_risk: samples of shape [K, S, 4]"),
             (lambda: m.cast_segments(t(5, 4)), samples % ("cast_segments", 8)), (lambda: m.grow_boxes(t(5, 9), (1, 1, 1)), samples % ("grow_boxes", 8)),
             (lambda: m.score_views(t(5, 8), 1), samples % ("score_views", 9)), (lambda: m.score_view_sets(t(5, 2, 8), 1), samples % ("score_view_sets", 9)),
             (lambda: m.score_view_sets(t(5, 9), 1), "score_view_sets: views of shape [n_sets, set_size, 9]"),
             (lambda: m.select_views(t(5, 8), 1, 1), samples % ("select_views", 9)), (lambda: m.select_views(t(5, 2, 9), 1, 1), "select_views: views of shape [n, 9]"),
             (lambda: m.build_reach_fields(t(5, 3)), points % "build_reach_fields"), (lambda: m.build_reach_timeline(t(5, 4, dtype=torch.float64)), points % "build_reach_fields"),
             (lambda: m.build_cost_fields(t(5, 5)), points % "build_cost_fields"), (lambda: m.reach_paths(t(5, 3), 4), points % "reach_paths"),
             (lambda: m.reach_timeline_paths(t(5, 4, dtype=torch.int64), 4), points % "reach_timeline_paths"), (lambda: m.cost_paths(t(5, 8), 4), points % "cost_paths")]
    both = "shorten_paths: int32 tensors steps [n] and cells [n, max_len] on one device"
    i32 = torch.int32
    cases += [(lambda: m.shorten_paths(t(5, dtype=i32), t(4, 6, dtype=i32)), both), (lambda: m.shorten_paths(t(5, dtype=i32), t(5, 6)), both),
              (lambda: m.shorten_paths(t(5), t(5, 6, dtype=i32)), both), (lambda: m.shorten_paths(t(5, dtype=i32), t(30, dtype=i32)), both),
              (lambda: m.shorten_paths(np.zeros(5, np.int32), t(5, 6, dtype=i32)), both)]
    for k, (call, text) in enumerate(cases):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == text, k


def test_empty_device_lists(env, dsp):
    """a build that keeps nothing: the device lists are empty int32 tensors of the host copies' column counts"""
    m = dsp.DSPMap(dsp.make_config(nx=SHAPE[0], ny=SHAPE[1], nz=SHAPE[2], res=RES, ppv=12, seed=7))
    m._chk(m.L.dspmap_init_device(m.h))
    m._chk(m.L.dspmap_set_stream(m.h, env.handle_stream.cuda_stream))
    pts = (common.wall_cloud(3, n_side=40) * F(0.6 / 3.0)).astype(F)
    with torch.cuda.stream(env.torch_stream):
        assert m.update(pts, env.cur, 0.0, QUATS[0]) == 1
        m.integrate_known()
        for f in (1, 2):                                  # two frames later nothing has age 0 any more: no cell is known at max_age 0
            assert m.update(pts, env.cur, f / 30.0, QUATS[0]) == 1
        m.build_cast_grid(env.thr, 0)
        m.build_frontiers(-1.0, 0, 1, 4)
        m.build_objects(-1.0, 26, 10 ** 6, 4096)          # no component has a million cells
        m.update_tracks(0.1)
        assert m.frontier_counts()[:2] == (0, 0) and m.object_counts()[0] == 0 and m.track_counts()[0] == 0
        for name, cols in (("frontier_cells", ()), ("frontier_blocks", (6,)), ("objects", (22,)), ("tracks", (18,))):
            host, dev = getattr(m, name)(), getattr(m, name)(device="cuda")
            assert len(host) == 0 and dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (0,) + cols, name
    m.close()
