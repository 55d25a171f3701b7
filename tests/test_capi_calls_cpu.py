"""CPU test of the binding's numpy call paths (dsp-map_amd/capi.py), without a device and without the library: a DSPMap made with
__new__ whose `L` is a recording stub.  Every wrapper of the planning layers -- the sample-taking ones, the layered host getters, the
counts readers and the two-call host lists -- is called over its input sizes, options and wrong shapes, and the list of library calls
it makes (symbol, arguments) and what it returns (dtype and shape) are compared with the literal TABLE below, which was recorded from
the binding before its wrappers were folded onto one call path.

In a recorded call an int, float or flag argument stands as its value, a pointer as None or 'ptr' (which of the two is the binding's
convention for empty inputs and optional outputs), a c_int passed by reference as 'ref'.  A result is 'f4[5]' for an array, a tuple of
those, an int, None, or the exception's type and text."""
import ctypes as C

import numpy as np
import pytest

import dsp_map_amd as D

capi = D.capi
F = np.float32
NX, NY, NZ, T, NP = 5, 4, 3, 2, 6


class Stub:
    """stands in for the loaded library: any attribute is a callable that records (symbol, normalised arguments) and returns `ret[symbol]`
    or `rc`; a c_int passed by reference is set to `entries`"""

    def __init__(self, rc=0, entries=0, fail=None):
        self.calls, self.rc, self.entries, self.fail = [], rc, entries, fail
        self.ret = {"dspmap_voxel_num": NX * NY * NZ, "dspmap_forecast_times": 3, "dspmap_last_error": b"stub error"}

    def __getattr__(self, name):
        argtypes = capi.SIGNATURES[name][1]   # (KeyError: the binding asked for a symbol the header does not declare)

        def fn(*args):
            assert len(args) == len(argtypes), (name, len(args))
            rec = []
            for a, t in zip(args, argtypes):
                if t in (C.c_int, C.c_uint):
                    assert isinstance(a, (int, np.integer)) and not isinstance(a, bool), (name, a)
                    rec.append(int(a))
                elif t in (C.c_float, C.c_double):
                    assert isinstance(a, float), (name, a)
                    rec.append(a)
                elif hasattr(a, "_obj"):   # C.byref(...)
                    assert isinstance(a._obj, C.c_int), (name, a)
                    a._obj.value = self.entries
                    rec.append("ref")
                else:                      # a pointer: None, a c_void_p, an address
                    v = a.value if isinstance(a, C.c_void_p) else a
                    assert v is None or isinstance(v, int), (name, a)
                    rec.append("ptr" if v else None)
            if name == "dspmap_build_cost_fields":   # (what the bands pointer holds)
                b = capi.CostBands.from_address(args[5])
                rec[5] = "bands(%d, %s, %s)" % (b.n_bands, [round(c, 2) for c in b.clearance], list(b.penalty))
            self.calls.append("%s(%s)" % (name, ", ".join(map(repr, rec))))
            if self.fail in (name, "*") and name not in ("dspmap_last_error", "dspmap_voxel_num"):
                return -1
            return self.ret.get(name, self.rc)
        return fn


def make_map(**stub):
    m = capi.DSPMap.__new__(capi.DSPMap)
    m.L = Stub(**stub)
    m.h = 1
    m.cfg = capi.make_config(nx=NX, ny=NY, nz=NZ, pred_times=(0.5, 1.0))
    m.T, m.NP, m.V = T, NP, NX * NY * NZ
    return m


def describe(r):
    if isinstance(r, np.ndarray):
        kind = r.dtype.str[1:] if r.dtype.names is None else [k for k, v in vars(capi).items() if k.endswith("_DTYPE") and v == r.dtype][0]
        return "%s%s" % (kind, list(r.shape))
    if isinstance(r, tuple):
        return "(" + ", ".join(describe(x) for x in r) + ")"
    assert r is None or type(r) is int, r
    return repr(r)


def f4(*shape):
    return np.arange(int(np.prod(shape)), dtype=F).reshape(shape)


def points(n, structured):
    if not structured:
        return f4(n, 4)
    p = np.zeros(n, capi.REACH_POINT_DTYPE)
    p["x"] = np.arange(n)
    return p


def cases():
    """[(id, call(m), stub options)]"""
    out = []

    def add(name, fn, **stub):
        out.append((name, fn, stub))

    for n in (0, 1, 5):
        q, s8, v9 = f4(n, 4), f4(n, 8), f4(n, 9)
        add("query_occupancy n=%d" % n, lambda m, q=q: m.query_occupancy(q))
        add("query_distance n=%d" % n, lambda m, q=q: m.query_distance(q))
        add("query_distance grad=False n=%d" % n, lambda m, q=q: m.query_distance(q, grad=False))
        add("query_forecast n=%d" % n, lambda m, q=q: m.query_forecast(q))
        add("query_known n=%d" % n, lambda m, q=q: m.query_known(q))
        add("query_objects n=%d" % n, lambda m, q=q: m.query_objects(q))
        add("trajectory_risk k=%d" % n, lambda m, n=n: m.trajectory_risk(f4(n, 3, 4)))
        add("cast_segments n=%d" % n, lambda m, s=s8: m.cast_segments(s))
        add("grow_boxes n=%d" % n, lambda m, s=s8: m.grow_boxes(s, (8, 8, 4)))
        add("score_views n=%d" % n, lambda m, v=v9: m.score_views(v, 7))
        add("select_views n=%d" % n, lambda m, v=v9: m.select_views(v, 3, 7))
        add("select_views scores n=%d" % n, lambda m, v=v9: m.select_views(v, 3, 7, n_fixed=1, min_gain=2, scores=True))
        add("score_view_sets n=%d" % n, lambda m, n=n: m.score_view_sets(f4(n, 2, 9), 7))
        add("score_view_sets scores n=%d" % n, lambda m, n=n: m.score_view_sets(f4(n, 2, 9), 7, scores=True))
        for structured in (False, True):
            p = points(n, structured)
            tag = "%s n=%d" % ("struct" if structured else "rows", n)
            add("build_reach_fields %s" % tag, lambda m, p=p: m.build_reach_fields(p, 2, t_start=0.5, step_seconds=0.1, max_steps=9))
            add("build_reach_timeline %s" % tag, lambda m, p=p: (m.build_reach_timeline(p, 2, max_steps=9), m._timeline_steps)[1])
            add("build_cost_fields %s" % tag, lambda m, p=p: m.build_cost_fields(p, 2, t=0.5, max_cost=99))
            for w in ("reach_paths", "reach_timeline_paths", "cost_paths"):
                add("%s %s" % (w, tag), lambda m, p=p, w=w: getattr(m, w)(p, 6))
                add("%s max_len=0 %s" % (w, tag), lambda m, p=p, w=w: getattr(m, w)(p, 0))
        for max_seg in (None, 0, 3):
            add("shorten_paths max_seg=%s n=%d" % (max_seg, n),
                lambda m, n=n, ms=max_seg: m.shorten_paths(np.zeros(n, np.int32), np.zeros((n, 6), np.int32), 0.5, 0.1, 8, ms))
        add("shorten_paths max_len=0 n=%d" % n, lambda m, n=n: m.shorten_paths(np.zeros(n, np.int32), np.zeros((n, 0), np.int32)))
        add("shorten_paths max_len=1 n=%d" % n, lambda m, n=n: m.shorten_paths(np.zeros((n, 1), np.int32), np.zeros((n, 1), np.int32)))
        add("build_forecast n=%d" % n, lambda m, n=n: m.build_forecast(np.arange(n)))
    # the flags
    q, s8, v9, p = f4(5, 4), f4(5, 8), f4(5, 9), points(5, False)
    add("query_occupancy world", lambda m: m.query_occupancy(q, radius=0.3, world=True, outside=0.5))
    add("trajectory_risk world", lambda m: m.trajectory_risk(f4(2, 3, 4), radius=0.3, world=True, outside=0.5, threshold=0.25))
    add("query_distance world", lambda m: m.query_distance(q, world=True, outside=2.0))
    add("query_forecast world", lambda m: m.query_forecast(q, world=True, outside=0.5))
    add("query_forecast lerp", lambda m: m.query_forecast(q, lerp=True))
    add("query_known world", lambda m: m.query_known(q, world=True))
    add("query_objects world", lambda m: m.query_objects(q, world=True))
    add("cast_segments world", lambda m: m.cast_segments(s8, world=True))
    add("grow_boxes world", lambda m: m.grow_boxes(s8, (1, 2, 3), world=True))
    add("grow_boxes with_current", lambda m: m.grow_boxes(s8, (1, 2, 3), with_current=True))
    add("score_views world", lambda m: m.score_views(v9, 7, world=True))
    add("score_view_sets world", lambda m: m.score_view_sets(f4(3, 2, 9), 7, world=True))
    add("select_views world", lambda m: m.select_views(v9, 3, 7, world=True))
    add("select_views k=0", lambda m: m.select_views(v9, 0, 7))
    add("select_views k=-1", lambda m: m.select_views(v9, -1, 7))
    for kw in (dict(world=True), dict(with_current=True), dict(device_sets=True), dict(world=True, with_current=True, device_sets=True)):
        tag = "+".join(sorted(kw))
        add("build_reach_fields %s" % tag, lambda m, kw=kw: m.build_reach_fields(p, **kw))
        add("build_reach_timeline %s" % tag, lambda m, kw=kw: m.build_reach_timeline(p, **kw))
    add("build_cost_fields world", lambda m: m.build_cost_fields(p, world=True))
    for nb in (0, 2, 5):
        add("build_cost_fields bands=%d" % nb, lambda m, nb=nb: m.build_cost_fields(p, bands=[(0.3 * (k + 1), k + 1) for k in range(nb)]))
    for w in ("reach_paths", "reach_timeline_paths", "cost_paths"):
        add("%s world" % w, lambda m, w=w: getattr(m, w)(p, 6, world=True))
        add("%s max_len=-1" % w, lambda m, w=w: getattr(m, w)(p, -1))
    add("build_reach_timeline then reach_sets", lambda m: (m.build_reach_timeline(p, max_steps=9), m.reach_sets(1))[1])
    add("build_reach_timeline then reach_sets first_step=4", lambda m: (m.build_reach_timeline(p, max_steps=9), m.reach_sets(1, first_step=4))[1])
    add("build_reach_timeline then reach_sets first_step=12", lambda m: (m.build_reach_timeline(p, max_steps=9), m.reach_sets(1, first_step=12))[1])
    add("reach_sets without a build", lambda m: m.reach_sets(0))
    add("reach_sets n_steps=3", lambda m: m.reach_sets(0, 2, 3))
    add("reach_sets n_steps=0", lambda m: m.reach_sets(0, 2, 0))
    add("reach_last_steps", lambda m: m.reach_last_steps(3))
    # the builds and whole-grid copies of the same sections
    add("build_distance_field", lambda m: m.build_distance_field(0.2, 8))
    add("build_distance_field outside_occupied", lambda m: m.build_distance_field(0.2, 8, outside_occupied=True))
    add("build_cast_grid", lambda m: m.build_cast_grid(0.2, 2))
    add("forecast_times", lambda m: m.forecast_times())
    add("cost_weights", lambda m: m.cost_weights())
    add("integrate_known", lambda m: m.integrate_known())
    add("integrate_known max_range", lambda m: m.integrate_known(2.5))
    add("reset_known", lambda m: m.reset_known())
    add("known_age", lambda m: m.known_age())
    add("mask_cast_grid", lambda m: m.mask_cast_grid(3))
    add("build_frontiers", lambda m: m.build_frontiers(0.5, 3, 2, 8))
    add("frontier_grid", lambda m: m.frontier_grid())
    add("build_objects", lambda m: m.build_objects(0.5, 6, 2, 100))
    add("object_labels", lambda m: m.object_labels())
    add("update_tracks", lambda m: m.update_tracks(0.1, 2, 4, 64, per_cell=True))
    add("reset_tracks", lambda m: m.reset_tracks())
    # the layered host getters
    for layer in (None, 1):
        add("distance_field layer=%s" % layer, lambda m, l=layer: m.distance_field(l))
        add("cast_grid layer=%s" % layer, lambda m, l=layer: m.cast_grid(l))
        add("forecast layer=%s" % layer, lambda m, l=layer: m.forecast(l))
    for w in ("reach_field", "cost_field"):
        add("%s field=1" % w, lambda m, w=w: getattr(m, w)(1))
        add("%s field=None n_fields=3" % w, lambda m, w=w: getattr(m, w)(None, 3))
        add("%s field=1 n_fields=3" % w, lambda m, w=w: getattr(m, w)(1, 3))
    # the counts readers
    add("reach_storage", lambda m: m.reach_storage())
    add("known_stats", lambda m: m.known_stats(4))
    add("object_counts", lambda m: m.object_counts())
    add("frontier_counts", lambda m: m.frontier_counts())
    add("track_counts", lambda m: m.track_counts())
    # the two-call host lists
    for w in ("frontier_cells", "frontier_blocks", "objects", "tracks"):
        for entries in (0, 3):
            add("%s entries=%d" % (w, entries), lambda m, w=w: getattr(m, w)(), entries=entries)
    # every shape error
    bad4, bad8, bad9 = f4(5, 3), f4(5, 4), f4(5, 8)
    for w in ("query_occupancy", "query_distance", "query_forecast", "query_known", "query_objects"):
        add("%s bad shape" % w, lambda m, w=w: getattr(m, w)(bad4))
        add("%s scalar" % w, lambda m, w=w: getattr(m, w)(1.0))
    add("trajectory_risk 2-d", lambda m: m.trajectory_risk(f4(5, 4)))
    add("trajectory_risk bad shape", lambda m: m.trajectory_risk(f4(5, 4, 3)))
    add("cast_segments bad shape", lambda m: m.cast_segments(bad8))
    add("grow_boxes bad shape", lambda m: m.grow_boxes(bad8, (1, 1, 1)))
    add("score_views bad shape", lambda m: m.score_views(bad9, 7))
    add("score_view_sets 2-d", lambda m: m.score_view_sets(f4(5, 9), 7))
    add("score_view_sets bad shape", lambda m: m.score_view_sets(f4(5, 2, 8), 7))
    add("select_views 3-d", lambda m: m.select_views(f4(5, 2, 9), 3, 7))
    add("select_views bad shape", lambda m: m.select_views(bad9, 3, 7))
    for w, call in (("build_reach_fields", lambda m, a: m.build_reach_fields(a)), ("build_reach_timeline", lambda m, a: m.build_reach_timeline(a)),
                    ("build_cost_fields", lambda m, a: m.build_cost_fields(a)), ("reach_paths", lambda m, a: m.reach_paths(a, 6)),
                    ("reach_timeline_paths", lambda m, a: m.reach_timeline_paths(a, 6)), ("cost_paths", lambda m, a: m.cost_paths(a, 6))):
        add("%s bad shape" % w, lambda m, call=call: call(m, bad4))
    add("shorten_paths 1-d cells", lambda m: m.shorten_paths(np.zeros(5, np.int32), np.zeros(5, np.int32)))
    add("shorten_paths steps too short", lambda m: m.shorten_paths(np.zeros(4, np.int32), np.zeros((5, 6), np.int32)))
    add("reach_field neither", lambda m: m.reach_field())
    add("cost_field neither", lambda m: m.cost_field())
    # a library error: -1 from the stub becomes DSPMapError with the stub's dspmap_last_error text
    for name, fn, stub in list(out):
        words = name.split(" ")
        if not stub and (words[1:] in ([], ["n=5"], ["k=5"], ["rows", "n=5"], ["layer=None"], ["field=1"]) or name == "shorten_paths max_seg=None n=5"):
            add(name + " !fails", fn, fail="*")
    for w, sym in (("frontier_cells", "dspmap_get_frontier_cells"), ("frontier_blocks", "dspmap_get_frontier_blocks"), ("objects", "dspmap_get_objects"),
                   ("tracks", "dspmap_get_tracks")):
        add("%s !fails" % w, lambda m, w=w: getattr(m, w)(), entries=3, fail=sym)
    add("forecast layer=None !get fails", lambda m: m.forecast(), fail="dspmap_get_forecast")
    return out


def record(fn, stub):
    m = make_map(**stub)
    try:
        result = describe(fn(m))
    except (ValueError, capi.DSPMapError) as e:
        result = "%s: %s" % (type(e).__name__, e)
    calls = m.L.calls
    m.h = None
    return calls, result


CASES = cases()


def test_table_covers_the_cases_and_the_wrappers():
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(TABLE)
    for w in ("query_occupancy", "trajectory_risk", "query_distance", "cast_segments", "grow_boxes", "build_reach_fields", "build_reach_timeline",
              "reach_paths", "reach_timeline_paths", "build_cost_fields", "cost_paths", "shorten_paths", "query_forecast", "query_known",
              "score_views", "score_view_sets", "select_views", "query_objects", "distance_field", "cast_grid", "forecast", "reach_field",
              "cost_field", "reach_storage", "known_stats", "object_counts", "frontier_counts", "track_counts", "frontier_cells",
              "frontier_blocks", "objects", "tracks"):
        mine = [i for i in ids if i.split(" ")[0] == w]
        assert mine and any("!fails" in i for i in mine), w
    errors = [v[1] for v in TABLE.values()]
    assert sum(e.startswith("ValueError: ") for e in errors) >= 25 and sum(e == "DSPMapError: stub error" for e in errors) >= 30


@pytest.mark.parametrize("name,fn,stub", CASES, ids=[c[0] for c in CASES])
def test_calls_and_results(name, fn, stub):
    calls, result = record(fn, stub)
    want_calls, want_result = TABLE[name]
    assert calls == want_calls
    assert result == want_result


# recorded from the binding as it was before the fold (see the module docstring)
TABLE = {
    'query_occupancy n=0': (["dspmap_query_occupancy('ptr', 0, 'ptr', 0.0, 0, 1.0, 'ptr')"], 'f4[0]'),
    'query_distance n=0': (["dspmap_query_distance('ptr', 0, 'ptr', 0, 0.0, 'ptr', 'ptr')"], '(f4[0], f4[0, 3])'),
    'query_distance grad=False n=0': (["dspmap_query_distance('ptr', 0, 'ptr', 0, 0.0, 'ptr', None)"], 'f4[0]'),
    'query_forecast n=0': (["dspmap_query_forecast('ptr', 0, 'ptr', 0, 1.0, 'ptr')"], 'f4[0]'),
    'query_known n=0': (["dspmap_query_known('ptr', 0, 'ptr', 0, 'ptr')"], 'i4[0]'),
    'query_objects n=0': (["dspmap_query_objects('ptr', 0, 'ptr', 0, 'ptr')"], 'i4[0]'),
    'trajectory_risk k=0': (["dspmap_trajectory_risk('ptr', 0, 3, 'ptr', 0.0, 0, 1.0, 0.5, 'ptr')"], 'RISK_DTYPE[0]'),
    'cast_segments n=0': (["dspmap_cast_segments('ptr', 0, 'ptr', 0, 'ptr')"], 'HIT_DTYPE[0]'),
    'grow_boxes n=0': (["dspmap_grow_boxes('ptr', 0, 'ptr', 'ptr', 0, 'ptr')"], 'BOX_DTYPE[0]'),
    'score_views n=0': (["dspmap_score_views('ptr', 0, 'ptr', 7, 0, 'ptr')"], 'VIEW_SCORE_DTYPE[0]'),
    'select_views n=0': (["dspmap_select_views('ptr', 0, 'ptr', 0, 7, 0, 3, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[3]'),
    'select_views scores n=0': (["dspmap_select_views('ptr', 0, 'ptr', 1, 7, 0, 3, 2, 'ptr', 'ptr')"], '(VIEW_PICK_DTYPE[3], VIEW_SCORE_DTYPE[0])'),
    'score_view_sets n=0': (["dspmap_score_view_sets('ptr', 0, 2, 'ptr', 7, 0, 'ptr', None)"], 'VIEW_SET_SCORE_DTYPE[0]'),
    'score_view_sets scores n=0': (["dspmap_score_view_sets('ptr', 0, 2, 'ptr', 7, 0, 'ptr', 'ptr')"], '(VIEW_SET_SCORE_DTYPE[0], VIEW_SCORE_DTYPE[0, 2])'),
    'build_reach_fields rows n=0': (["dspmap_build_reach_fields('ptr', 2, 0, None, 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline rows n=0': (["dspmap_build_reach_timeline('ptr', 2, 0, None, -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields rows n=0': (["dspmap_build_cost_fields('ptr', 2, 0, None, 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths rows n=0': (["dspmap_reach_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'reach_paths max_len=0 rows n=0': (["dspmap_reach_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'reach_timeline_paths rows n=0': (["dspmap_reach_timeline_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'reach_timeline_paths max_len=0 rows n=0': (["dspmap_reach_timeline_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'cost_paths rows n=0': (["dspmap_cost_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'cost_paths max_len=0 rows n=0': (["dspmap_cost_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'build_reach_fields struct n=0': (["dspmap_build_reach_fields('ptr', 2, 0, None, 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline struct n=0': (["dspmap_build_reach_timeline('ptr', 2, 0, None, -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields struct n=0': (["dspmap_build_cost_fields('ptr', 2, 0, None, 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths struct n=0': (["dspmap_reach_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'reach_paths max_len=0 struct n=0': (["dspmap_reach_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'reach_timeline_paths struct n=0': (["dspmap_reach_timeline_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'reach_timeline_paths max_len=0 struct n=0': (["dspmap_reach_timeline_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'cost_paths struct n=0': (["dspmap_cost_paths('ptr', 0, None, 6, 0, None, 'ptr')"], '(i4[0], i4[0, 6])'),
    'cost_paths max_len=0 struct n=0': (["dspmap_cost_paths('ptr', 0, None, 0, 0, None, None)"], '(i4[0], i4[0, 0])'),
    'shorten_paths max_seg=None n=0': (["dspmap_shorten_paths('ptr', 0, 6, None, None, 0.5, 0.1, 8, 5, 0, None, None, None)"], '(PATH_INFO_DTYPE[0], f4[0, 5, 8], i4[0, 5])'),
    'shorten_paths max_seg=0 n=0': (["dspmap_shorten_paths('ptr', 0, 6, None, None, 0.5, 0.1, 8, 0, 0, None, None, None)"], '(PATH_INFO_DTYPE[0], f4[0, 0, 8], i4[0, 0])'),
    'shorten_paths max_seg=3 n=0': (["dspmap_shorten_paths('ptr', 0, 6, None, None, 0.5, 0.1, 8, 3, 0, None, None, None)"], '(PATH_INFO_DTYPE[0], f4[0, 3, 8], i4[0, 3])'),
    'shorten_paths max_len=0 n=0': (["dspmap_shorten_paths('ptr', 0, 0, None, None, -1.0, 0.0, 64, 0, 0, None, None, None)"], '(PATH_INFO_DTYPE[0], f4[0, 0, 8], i4[0, 0])'),
    'shorten_paths max_len=1 n=0': (["dspmap_shorten_paths('ptr', 0, 1, None, None, -1.0, 0.0, 64, 0, 0, None, None, None)"], '(PATH_INFO_DTYPE[0], f4[0, 0, 8], i4[0, 0])'),
    'build_forecast n=0': (["dspmap_build_forecast('ptr', 0, None, 0)"], 'None'),
    'query_occupancy n=1': (["dspmap_query_occupancy('ptr', 1, 'ptr', 0.0, 0, 1.0, 'ptr')"], 'f4[1]'),
    'query_distance n=1': (["dspmap_query_distance('ptr', 1, 'ptr', 0, 0.0, 'ptr', 'ptr')"], '(f4[1], f4[1, 3])'),
    'query_distance grad=False n=1': (["dspmap_query_distance('ptr', 1, 'ptr', 0, 0.0, 'ptr', None)"], 'f4[1]'),
    'query_forecast n=1': (["dspmap_query_forecast('ptr', 1, 'ptr', 0, 1.0, 'ptr')"], 'f4[1]'),
    'query_known n=1': (["dspmap_query_known('ptr', 1, 'ptr', 0, 'ptr')"], 'i4[1]'),
    'query_objects n=1': (["dspmap_query_objects('ptr', 1, 'ptr', 0, 'ptr')"], 'i4[1]'),
    'trajectory_risk k=1': (["dspmap_trajectory_risk('ptr', 1, 3, 'ptr', 0.0, 0, 1.0, 0.5, 'ptr')"], 'RISK_DTYPE[1]'),
    'cast_segments n=1': (["dspmap_cast_segments('ptr', 1, 'ptr', 0, 'ptr')"], 'HIT_DTYPE[1]'),
    'grow_boxes n=1': (["dspmap_grow_boxes('ptr', 1, 'ptr', 'ptr', 0, 'ptr')"], 'BOX_DTYPE[1]'),
    'score_views n=1': (["dspmap_score_views('ptr', 1, 'ptr', 7, 0, 'ptr')"], 'VIEW_SCORE_DTYPE[1]'),
    'select_views n=1': (["dspmap_select_views('ptr', 1, 'ptr', 0, 7, 0, 3, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[3]'),
    'select_views scores n=1': (["dspmap_select_views('ptr', 1, 'ptr', 1, 7, 0, 3, 2, 'ptr', 'ptr')"], '(VIEW_PICK_DTYPE[3], VIEW_SCORE_DTYPE[1])'),
    'score_view_sets n=1': (["dspmap_score_view_sets('ptr', 1, 2, 'ptr', 7, 0, 'ptr', None)"], 'VIEW_SET_SCORE_DTYPE[1]'),
    'score_view_sets scores n=1': (["dspmap_score_view_sets('ptr', 1, 2, 'ptr', 7, 0, 'ptr', 'ptr')"], '(VIEW_SET_SCORE_DTYPE[1], VIEW_SCORE_DTYPE[1, 2])'),
    'build_reach_fields rows n=1': (["dspmap_build_reach_fields('ptr', 2, 1, 'ptr', 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline rows n=1': (["dspmap_build_reach_timeline('ptr', 2, 1, 'ptr', -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields rows n=1': (["dspmap_build_cost_fields('ptr', 2, 1, 'ptr', 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths rows n=1': (["dspmap_reach_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'reach_paths max_len=0 rows n=1': (["dspmap_reach_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'reach_timeline_paths rows n=1': (["dspmap_reach_timeline_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'reach_timeline_paths max_len=0 rows n=1': (["dspmap_reach_timeline_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'cost_paths rows n=1': (["dspmap_cost_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'cost_paths max_len=0 rows n=1': (["dspmap_cost_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'build_reach_fields struct n=1': (["dspmap_build_reach_fields('ptr', 2, 1, 'ptr', 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline struct n=1': (["dspmap_build_reach_timeline('ptr', 2, 1, 'ptr', -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields struct n=1': (["dspmap_build_cost_fields('ptr', 2, 1, 'ptr', 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths struct n=1': (["dspmap_reach_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'reach_paths max_len=0 struct n=1': (["dspmap_reach_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'reach_timeline_paths struct n=1': (["dspmap_reach_timeline_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'reach_timeline_paths max_len=0 struct n=1': (["dspmap_reach_timeline_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'cost_paths struct n=1': (["dspmap_cost_paths('ptr', 1, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[1], i4[1, 6])'),
    'cost_paths max_len=0 struct n=1': (["dspmap_cost_paths('ptr', 1, 'ptr', 0, 0, 'ptr', None)"], '(i4[1], i4[1, 0])'),
    'shorten_paths max_seg=None n=1': (["dspmap_shorten_paths('ptr', 1, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 5, 0, 'ptr', 'ptr', 'ptr')"], '(PATH_INFO_DTYPE[1], f4[1, 5, 8], i4[1, 5])'),
    'shorten_paths max_seg=0 n=1': (["dspmap_shorten_paths('ptr', 1, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[1], f4[1, 0, 8], i4[1, 0])'),
    'shorten_paths max_seg=3 n=1': (["dspmap_shorten_paths('ptr', 1, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 3, 0, 'ptr', 'ptr', 'ptr')"], '(PATH_INFO_DTYPE[1], f4[1, 3, 8], i4[1, 3])'),
    'shorten_paths max_len=0 n=1': (["dspmap_shorten_paths('ptr', 1, 0, 'ptr', 'ptr', -1.0, 0.0, 64, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[1], f4[1, 0, 8], i4[1, 0])'),
    'shorten_paths max_len=1 n=1': (["dspmap_shorten_paths('ptr', 1, 1, 'ptr', 'ptr', -1.0, 0.0, 64, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[1], f4[1, 0, 8], i4[1, 0])'),
    'build_forecast n=1': (["dspmap_build_forecast('ptr', 1, 'ptr', 0)"], 'None'),
    'query_occupancy n=5': (["dspmap_query_occupancy('ptr', 5, 'ptr', 0.0, 0, 1.0, 'ptr')"], 'f4[5]'),
    'query_distance n=5': (["dspmap_query_distance('ptr', 5, 'ptr', 0, 0.0, 'ptr', 'ptr')"], '(f4[5], f4[5, 3])'),
    'query_distance grad=False n=5': (["dspmap_query_distance('ptr', 5, 'ptr', 0, 0.0, 'ptr', None)"], 'f4[5]'),
    'query_forecast n=5': (["dspmap_query_forecast('ptr', 5, 'ptr', 0, 1.0, 'ptr')"], 'f4[5]'),
    'query_known n=5': (["dspmap_query_known('ptr', 5, 'ptr', 0, 'ptr')"], 'i4[5]'),
    'query_objects n=5': (["dspmap_query_objects('ptr', 5, 'ptr', 0, 'ptr')"], 'i4[5]'),
    'trajectory_risk k=5': (["dspmap_trajectory_risk('ptr', 5, 3, 'ptr', 0.0, 0, 1.0, 0.5, 'ptr')"], 'RISK_DTYPE[5]'),
    'cast_segments n=5': (["dspmap_cast_segments('ptr', 5, 'ptr', 0, 'ptr')"], 'HIT_DTYPE[5]'),
    'grow_boxes n=5': (["dspmap_grow_boxes('ptr', 5, 'ptr', 'ptr', 0, 'ptr')"], 'BOX_DTYPE[5]'),
    'score_views n=5': (["dspmap_score_views('ptr', 5, 'ptr', 7, 0, 'ptr')"], 'VIEW_SCORE_DTYPE[5]'),
    'select_views n=5': (["dspmap_select_views('ptr', 5, 'ptr', 0, 7, 0, 3, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[3]'),
    'select_views scores n=5': (["dspmap_select_views('ptr', 5, 'ptr', 1, 7, 0, 3, 2, 'ptr', 'ptr')"], '(VIEW_PICK_DTYPE[3], VIEW_SCORE_DTYPE[5])'),
    'score_view_sets n=5': (["dspmap_score_view_sets('ptr', 5, 2, 'ptr', 7, 0, 'ptr', None)"], 'VIEW_SET_SCORE_DTYPE[5]'),
    'score_view_sets scores n=5': (["dspmap_score_view_sets('ptr', 5, 2, 'ptr', 7, 0, 'ptr', 'ptr')"], '(VIEW_SET_SCORE_DTYPE[5], VIEW_SCORE_DTYPE[5, 2])'),
    'build_reach_fields rows n=5': (["dspmap_build_reach_fields('ptr', 2, 5, 'ptr', 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline rows n=5': (["dspmap_build_reach_timeline('ptr', 2, 5, 'ptr', -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields rows n=5': (["dspmap_build_cost_fields('ptr', 2, 5, 'ptr', 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths rows n=5': (["dspmap_reach_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_paths max_len=0 rows n=5': (["dspmap_reach_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'reach_timeline_paths rows n=5': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_timeline_paths max_len=0 rows n=5': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'cost_paths rows n=5': (["dspmap_cost_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'cost_paths max_len=0 rows n=5': (["dspmap_cost_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'build_reach_fields struct n=5': (["dspmap_build_reach_fields('ptr', 2, 5, 'ptr', 0.5, 0.1, 9, 0)"], 'None'),
    'build_reach_timeline struct n=5': (["dspmap_build_reach_timeline('ptr', 2, 5, 'ptr', -1.0, 0.0, 9, 0)"], '9'),
    'build_cost_fields struct n=5': (["dspmap_build_cost_fields('ptr', 2, 5, 'ptr', 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)"], 'None'),
    'reach_paths struct n=5': (["dspmap_reach_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_paths max_len=0 struct n=5': (["dspmap_reach_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'reach_timeline_paths struct n=5': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_timeline_paths max_len=0 struct n=5': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'cost_paths struct n=5': (["dspmap_cost_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'cost_paths max_len=0 struct n=5': (["dspmap_cost_paths('ptr', 5, 'ptr', 0, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'shorten_paths max_seg=None n=5': (["dspmap_shorten_paths('ptr', 5, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 5, 0, 'ptr', 'ptr', 'ptr')"], '(PATH_INFO_DTYPE[5], f4[5, 5, 8], i4[5, 5])'),
    'shorten_paths max_seg=0 n=5': (["dspmap_shorten_paths('ptr', 5, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[5], f4[5, 0, 8], i4[5, 0])'),
    'shorten_paths max_seg=3 n=5': (["dspmap_shorten_paths('ptr', 5, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 3, 0, 'ptr', 'ptr', 'ptr')"], '(PATH_INFO_DTYPE[5], f4[5, 3, 8], i4[5, 3])'),
    'shorten_paths max_len=0 n=5': (["dspmap_shorten_paths('ptr', 5, 0, 'ptr', 'ptr', -1.0, 0.0, 64, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[5], f4[5, 0, 8], i4[5, 0])'),
    'shorten_paths max_len=1 n=5': (["dspmap_shorten_paths('ptr', 5, 1, 'ptr', 'ptr', -1.0, 0.0, 64, 0, 0, 'ptr', None, None)"], '(PATH_INFO_DTYPE[5], f4[5, 0, 8], i4[5, 0])'),
    'build_forecast n=5': (["dspmap_build_forecast('ptr', 5, 'ptr', 0)"], 'None'),
    'query_occupancy world': (["dspmap_query_occupancy('ptr', 5, 'ptr', 0.3, 1, 0.5, 'ptr')"], 'f4[5]'),
    'trajectory_risk world': (["dspmap_trajectory_risk('ptr', 2, 3, 'ptr', 0.3, 1, 0.5, 0.25, 'ptr')"], 'RISK_DTYPE[2]'),
    'query_distance world': (["dspmap_query_distance('ptr', 5, 'ptr', 1, 2.0, 'ptr', 'ptr')"], '(f4[5], f4[5, 3])'),
    'query_forecast world': (["dspmap_query_forecast('ptr', 5, 'ptr', 1, 0.5, 'ptr')"], 'f4[5]'),
    'query_forecast lerp': (["dspmap_query_forecast('ptr', 5, 'ptr', 2, 1.0, 'ptr')"], 'f4[5]'),
    'query_known world': (["dspmap_query_known('ptr', 5, 'ptr', 1, 'ptr')"], 'i4[5]'),
    'query_objects world': (["dspmap_query_objects('ptr', 5, 'ptr', 1, 'ptr')"], 'i4[5]'),
    'cast_segments world': (["dspmap_cast_segments('ptr', 5, 'ptr', 1, 'ptr')"], 'HIT_DTYPE[5]'),
    'grow_boxes world': (["dspmap_grow_boxes('ptr', 5, 'ptr', 'ptr', 1, 'ptr')"], 'BOX_DTYPE[5]'),
    'grow_boxes with_current': (["dspmap_grow_boxes('ptr', 5, 'ptr', 'ptr', 2, 'ptr')"], 'BOX_DTYPE[5]'),
    'score_views world': (["dspmap_score_views('ptr', 5, 'ptr', 7, 1, 'ptr')"], 'VIEW_SCORE_DTYPE[5]'),
    'score_view_sets world': (["dspmap_score_view_sets('ptr', 3, 2, 'ptr', 7, 1, 'ptr', None)"], 'VIEW_SET_SCORE_DTYPE[3]'),
    'select_views world': (["dspmap_select_views('ptr', 5, 'ptr', 0, 7, 1, 3, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[3]'),
    'select_views k=0': (["dspmap_select_views('ptr', 5, 'ptr', 0, 7, 0, 0, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[0]'),
    'select_views k=-1': (["dspmap_select_views('ptr', 5, 'ptr', 0, 7, 0, -1, 1, 'ptr', None)"], 'VIEW_PICK_DTYPE[0]'),
    'build_reach_fields world': (["dspmap_build_reach_fields('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 1)"], 'None'),
    'build_reach_timeline world': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 1)"], 'None'),
    'build_reach_fields with_current': (["dspmap_build_reach_fields('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 2)"], 'None'),
    'build_reach_timeline with_current': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 2)"], 'None'),
    'build_reach_fields device_sets': (["dspmap_build_reach_fields('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 4)"], 'None'),
    'build_reach_timeline device_sets': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 4)"], 'None'),
    'build_reach_fields device_sets+with_current+world': (["dspmap_build_reach_fields('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 7)"], 'None'),
    'build_reach_timeline device_sets+with_current+world': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 4096, 7)"], 'None'),
    'build_cost_fields world': (["dspmap_build_cost_fields('ptr', 1, 5, 'ptr', -1.0, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 16384, 1)"], 'None'),
    'build_cost_fields bands=0': (["dspmap_build_cost_fields('ptr', 1, 5, 'ptr', -1.0, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 16384, 0)"], 'None'),
    'build_cost_fields bands=2': (["dspmap_build_cost_fields('ptr', 1, 5, 'ptr', -1.0, 'bands(2, [0.3, 0.6, 0.0, 0.0], [1, 2, 0, 0])', 16384, 0)"], 'None'),
    'build_cost_fields bands=5': (["dspmap_build_cost_fields('ptr', 1, 5, 'ptr', -1.0, 'bands(5, [0.3, 0.6, 0.9, 1.2], [1, 2, 3, 4])', 16384, 0)"], 'None'),
    'reach_paths world': (["dspmap_reach_paths('ptr', 5, 'ptr', 6, 1, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_paths max_len=-1': (["dspmap_reach_paths('ptr', 5, 'ptr', -1, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'reach_timeline_paths world': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 6, 1, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'reach_timeline_paths max_len=-1': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', -1, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'cost_paths world': (["dspmap_cost_paths('ptr', 5, 'ptr', 6, 1, 'ptr', 'ptr')"], '(i4[5], i4[5, 6])'),
    'cost_paths max_len=-1': (["dspmap_cost_paths('ptr', 5, 'ptr', -1, 0, 'ptr', None)"], '(i4[5], i4[5, 0])'),
    'build_reach_timeline then reach_sets': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 9, 0)", "dspmap_get_reach_sets('ptr', 1, 0, 10, 'ptr')"], 'u8[10, 3, 4, 1]'),
    'build_reach_timeline then reach_sets first_step=4': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 9, 0)", "dspmap_get_reach_sets('ptr', 1, 4, 6, 'ptr')"], 'u8[6, 3, 4, 1]'),
    'build_reach_timeline then reach_sets first_step=12': (["dspmap_build_reach_timeline('ptr', 1, 5, 'ptr', -1.0, 0.0, 9, 0)", "dspmap_get_reach_sets('ptr', 1, 12, 0, None)"], 'u8[0, 3, 4, 1]'),
    'reach_sets without a build': (["dspmap_get_reach_sets('ptr', 0, 0, 1, 'ptr')"], 'u8[1, 3, 4, 1]'),
    'reach_sets n_steps=3': (["dspmap_get_reach_sets('ptr', 0, 2, 3, 'ptr')"], 'u8[3, 3, 4, 1]'),
    'reach_sets n_steps=0': (["dspmap_get_reach_sets('ptr', 0, 2, 0, None)"], 'u8[0, 3, 4, 1]'),
    'reach_last_steps': (["dspmap_reach_last_steps('ptr', 'ptr')"], 'i4[3]'),
    'build_distance_field': (["dspmap_build_distance_field('ptr', 0.2, 8, 0)"], 'None'),
    'build_distance_field outside_occupied': (["dspmap_build_distance_field('ptr', 0.2, 8, 1)"], 'None'),
    'build_cast_grid': (["dspmap_build_cast_grid('ptr', 0.2, 2, 0)"], 'None'),
    'forecast_times': (["dspmap_forecast_times('ptr', 'ptr', 64)"], 'f4[3]'),
    'cost_weights': (["dspmap_get_cost_weights('ptr', 'ptr')"], 'u1[3, 4, 5]'),
    'integrate_known': (["dspmap_known_integrate('ptr', inf, 0)"], 'None'),
    'integrate_known max_range': (["dspmap_known_integrate('ptr', 2.5, 0)"], 'None'),
    'reset_known': (["dspmap_known_reset('ptr')"], 'None'),
    'known_age': (["dspmap_get_known('ptr', 'ptr')"], 'i4[3, 4, 5]'),
    'mask_cast_grid': (["dspmap_mask_cast_grid('ptr', 3, 0)"], 'None'),
    'build_frontiers': (["dspmap_build_frontiers('ptr', 0.5, 3, 2, 8, 0)"], 'None'),
    'frontier_grid': (["dspmap_get_frontier_grid('ptr', 'ptr')"], 'u8[3, 4, 1]'),
    'build_objects': (["dspmap_build_objects('ptr', 0.5, 6, 2, 100, 0)"], 'None'),
    'object_labels': (["dspmap_get_object_labels('ptr', 'ptr')"], 'i4[3, 4, 5]'),
    'update_tracks': (["dspmap_track_update('ptr', 0.1, 2, 4, 64, 1)"], 'None'),
    'reset_tracks': (["dspmap_track_reset('ptr')"], 'None'),
    'distance_field layer=None': (["dspmap_get_distance_field('ptr', 0, 'ptr')", "dspmap_get_distance_field('ptr', 1, 'ptr')", "dspmap_get_distance_field('ptr', 2, 'ptr')"], 'f4[3, 3, 4, 5]'),
    'cast_grid layer=None': (["dspmap_get_cast_grid('ptr', 0, 'ptr')", "dspmap_get_cast_grid('ptr', 1, 'ptr')", "dspmap_get_cast_grid('ptr', 2, 'ptr')"], 'u8[3, 3, 4, 1]'),
    'forecast layer=None': (["dspmap_voxel_num('ptr')", "dspmap_forecast_times('ptr', 'ptr', 64)", "dspmap_get_forecast('ptr', 0, 'ptr')", "dspmap_get_forecast('ptr', 1, 'ptr')", "dspmap_get_forecast('ptr', 2, 'ptr')"], 'f4[3, 60]'),
    'distance_field layer=1': (["dspmap_get_distance_field('ptr', 1, 'ptr')"], 'f4[3, 4, 5]'),
    'cast_grid layer=1': (["dspmap_get_cast_grid('ptr', 1, 'ptr')"], 'u8[3, 4, 1]'),
    'forecast layer=1': (["dspmap_voxel_num('ptr')", "dspmap_get_forecast('ptr', 1, 'ptr')"], 'f4[60]'),
    'reach_field field=1': (["dspmap_get_reach_field('ptr', 1, 'ptr')"], 'u2[3, 4, 5]'),
    'reach_field field=None n_fields=3': (["dspmap_get_reach_field('ptr', 0, 'ptr')", "dspmap_get_reach_field('ptr', 1, 'ptr')", "dspmap_get_reach_field('ptr', 2, 'ptr')"], 'u2[3, 3, 4, 5]'),
    'reach_field field=1 n_fields=3': (["dspmap_get_reach_field('ptr', 1, 'ptr')"], 'u2[3, 4, 5]'),
    'cost_field field=1': (["dspmap_get_cost_field('ptr', 1, 'ptr')"], 'u2[3, 4, 5]'),
    'cost_field field=None n_fields=3': (["dspmap_get_cost_field('ptr', 0, 'ptr')", "dspmap_get_cost_field('ptr', 1, 'ptr')", "dspmap_get_cost_field('ptr', 2, 'ptr')"], 'u2[3, 3, 4, 5]'),
    'cost_field field=1 n_fields=3': (["dspmap_get_cost_field('ptr', 1, 'ptr')"], 'u2[3, 4, 5]'),
    'reach_storage': (["dspmap_debug_reach_storage('ptr', 'ptr')"], '(0, 0)'),
    'known_stats': (["dspmap_known_stats('ptr', 4, 'ptr')"], '(0, 0)'),
    'object_counts': (["dspmap_object_counts('ptr', 'ptr')"], '(0, 0, 0)'),
    'frontier_counts': (["dspmap_frontier_counts('ptr', 'ptr')"], '(0, 0, 0)'),
    'track_counts': (["dspmap_track_counts('ptr', 'ptr')"], '(0, 0, 0, 0, 0, 0)'),
    'frontier_cells entries=0': (["dspmap_get_frontier_cells('ptr', 0, None, 'ref')"], 'i4[0]'),
    'frontier_cells entries=3': (["dspmap_get_frontier_cells('ptr', 0, None, 'ref')", "dspmap_get_frontier_cells('ptr', 3, 'ptr', 'ref')"], 'i4[3]'),
    'frontier_blocks entries=0': (["dspmap_get_frontier_blocks('ptr', 0, None, 'ref')"], 'FRONTIER_BLOCK_DTYPE[0]'),
    'frontier_blocks entries=3': (["dspmap_get_frontier_blocks('ptr', 0, None, 'ref')", "dspmap_get_frontier_blocks('ptr', 3, 'ptr', 'ref')"], 'FRONTIER_BLOCK_DTYPE[3]'),
    'objects entries=0': (["dspmap_get_objects('ptr', 0, None, 'ref')"], 'OBJECT_DTYPE[0]'),
    'objects entries=3': (["dspmap_get_objects('ptr', 0, None, 'ref')", "dspmap_get_objects('ptr', 3, 'ptr', 'ref')"], 'OBJECT_DTYPE[3]'),
    'tracks entries=0': (["dspmap_get_tracks('ptr', 0, None, 'ref')"], 'TRACK_DTYPE[0]'),
    'tracks entries=3': (["dspmap_get_tracks('ptr', 0, None, 'ref')", "dspmap_get_tracks('ptr', 3, 'ptr', 'ref')"], 'TRACK_DTYPE[3]'),
    'query_occupancy bad shape': ([], 'ValueError: query_occupancy: samples of shape [n, 4]'),
    'query_occupancy scalar': ([], 'ValueError: query_occupancy: samples of shape [n, 4]'),
    'query_distance bad shape': ([], 'ValueError: query_distance: samples of shape [n, 4]'),
    'query_distance scalar': ([], 'ValueError: query_distance: samples of shape [n, 4]'),
    'query_forecast bad shape': ([], 'ValueError: query_forecast: samples of shape [n, 4]'),
    'query_forecast scalar': ([], 'ValueError: query_forecast: samples of shape [n, 4]'),
    'query_known bad shape': ([], 'ValueError: query_known: samples of shape [n, 4]'),
    'query_known scalar': ([], 'ValueError: query_known: samples of shape [n, 4]'),
    'query_objects bad shape': ([], 'ValueError: query_objects: samples of shape [n, 4]'),
    'query_objects scalar': ([], 'ValueError: query_objects: samples of shape [n, 4]'),
    'trajectory_risk 2-d': ([], 'ValueError: trajectory_risk: samples of shape [K, S, 4]'),
    'trajectory_risk bad shape': ([], 'ValueError: trajectory_risk: samples of shape [K, S, 4]'),
    'cast_segments bad shape': ([], 'ValueError: cast_segments: segments of shape [n, 8]'),
    'grow_boxes bad shape': ([], 'ValueError: grow_boxes: seeds of shape [n, 8]'),
    'score_views bad shape': ([], 'ValueError: score_views: views of shape [n, 9]'),
    'score_view_sets 2-d': ([], 'ValueError: score_view_sets: views of shape [n_sets, set_size, 9]'),
    'score_view_sets bad shape': ([], 'ValueError: score_view_sets: views of shape [n_sets, set_size, 9]'),
    'select_views 3-d': ([], 'ValueError: select_views: views of shape [n, 9]'),
    'select_views bad shape': ([], 'ValueError: select_views: views of shape [n, 9]'),
    'build_reach_fields bad shape': ([], 'ValueError: build_reach_fields: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'build_reach_timeline bad shape': ([], 'ValueError: build_reach_fields: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'build_cost_fields bad shape': ([], 'ValueError: build_cost_fields: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'reach_paths bad shape': ([], 'ValueError: reach_paths: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'reach_timeline_paths bad shape': ([], 'ValueError: reach_timeline_paths: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'cost_paths bad shape': ([], 'ValueError: cost_paths: points of shape [n, 4] or of REACH_POINT_DTYPE'),
    'shorten_paths 1-d cells': ([], 'ValueError: shorten_paths: steps [n] and cells [n, max_len]'),
    'shorten_paths steps too short': ([], 'ValueError: shorten_paths: steps [n] and cells [n, max_len]'),
    'reach_field neither': ([], 'ValueError: reach_field: a field, or n_fields for all of them'),
    'cost_field neither': ([], 'ValueError: cost_field: a field, or n_fields for all of them'),
    'query_occupancy n=5 !fails': (["dspmap_query_occupancy('ptr', 5, 'ptr', 0.0, 0, 1.0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'query_distance n=5 !fails': (["dspmap_query_distance('ptr', 5, 'ptr', 0, 0.0, 'ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'query_forecast n=5 !fails': (["dspmap_query_forecast('ptr', 5, 'ptr', 0, 1.0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'query_known n=5 !fails': (["dspmap_query_known('ptr', 5, 'ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'query_objects n=5 !fails': (["dspmap_query_objects('ptr', 5, 'ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'trajectory_risk k=5 !fails': (["dspmap_trajectory_risk('ptr', 5, 3, 'ptr', 0.0, 0, 1.0, 0.5, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'cast_segments n=5 !fails': (["dspmap_cast_segments('ptr', 5, 'ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'grow_boxes n=5 !fails': (["dspmap_grow_boxes('ptr', 5, 'ptr', 'ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'score_views n=5 !fails': (["dspmap_score_views('ptr', 5, 'ptr', 7, 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'select_views n=5 !fails': (["dspmap_select_views('ptr', 5, 'ptr', 0, 7, 0, 3, 1, 'ptr', None)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'score_view_sets n=5 !fails': (["dspmap_score_view_sets('ptr', 5, 2, 'ptr', 7, 0, 'ptr', None)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_reach_fields rows n=5 !fails': (["dspmap_build_reach_fields('ptr', 2, 5, 'ptr', 0.5, 0.1, 9, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_reach_timeline rows n=5 !fails': (["dspmap_build_reach_timeline('ptr', 2, 5, 'ptr', -1.0, 0.0, 9, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_cost_fields rows n=5 !fails': (["dspmap_build_cost_fields('ptr', 2, 5, 'ptr', 0.5, 'bands(0, [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0])', 99, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reach_paths rows n=5 !fails': (["dspmap_reach_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reach_timeline_paths rows n=5 !fails': (["dspmap_reach_timeline_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'cost_paths rows n=5 !fails': (["dspmap_cost_paths('ptr', 5, 'ptr', 6, 0, 'ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'shorten_paths max_seg=None n=5 !fails': (["dspmap_shorten_paths('ptr', 5, 6, 'ptr', 'ptr', 0.5, 0.1, 8, 5, 0, 'ptr', 'ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_forecast n=5 !fails': (["dspmap_build_forecast('ptr', 5, 'ptr', 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reach_last_steps !fails': (["dspmap_reach_last_steps('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_distance_field !fails': (["dspmap_build_distance_field('ptr', 0.2, 8, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_cast_grid !fails': (["dspmap_build_cast_grid('ptr', 0.2, 2, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'forecast_times !fails': (["dspmap_forecast_times('ptr', 'ptr', 64)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'cost_weights !fails': (["dspmap_get_cost_weights('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'integrate_known !fails': (["dspmap_known_integrate('ptr', inf, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reset_known !fails': (["dspmap_known_reset('ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'known_age !fails': (["dspmap_get_known('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'mask_cast_grid !fails': (["dspmap_mask_cast_grid('ptr', 3, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_frontiers !fails': (["dspmap_build_frontiers('ptr', 0.5, 3, 2, 8, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'frontier_grid !fails': (["dspmap_get_frontier_grid('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'build_objects !fails': (["dspmap_build_objects('ptr', 0.5, 6, 2, 100, 0)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'object_labels !fails': (["dspmap_get_object_labels('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'update_tracks !fails': (["dspmap_track_update('ptr', 0.1, 2, 4, 64, 1)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reset_tracks !fails': (["dspmap_track_reset('ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'distance_field layer=None !fails': (["dspmap_get_distance_field('ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'cast_grid layer=None !fails': (["dspmap_get_cast_grid('ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'forecast layer=None !fails': (["dspmap_voxel_num('ptr')", "dspmap_forecast_times('ptr', 'ptr', 64)", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reach_field field=1 !fails': (["dspmap_get_reach_field('ptr', 1, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'cost_field field=1 !fails': (["dspmap_get_cost_field('ptr', 1, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'reach_storage !fails': (["dspmap_debug_reach_storage('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'known_stats !fails': (["dspmap_known_stats('ptr', 4, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'object_counts !fails': (["dspmap_object_counts('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'frontier_counts !fails': (["dspmap_frontier_counts('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'track_counts !fails': (["dspmap_track_counts('ptr', 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'frontier_cells !fails': (["dspmap_get_frontier_cells('ptr', 0, None, 'ref')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'frontier_blocks !fails': (["dspmap_get_frontier_blocks('ptr', 0, None, 'ref')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'objects !fails': (["dspmap_get_objects('ptr', 0, None, 'ref')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'tracks !fails': (["dspmap_get_tracks('ptr', 0, None, 'ref')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
    'forecast layer=None !get fails': (["dspmap_voxel_num('ptr')", "dspmap_forecast_times('ptr', 'ptr', 64)", "dspmap_get_forecast('ptr', 0, 'ptr')", "dspmap_last_error('ptr')"], 'DSPMapError: stub error'),
}
