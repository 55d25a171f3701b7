"""Timing of the clearance-weighted cost-to-go fields (dspmap_build_cost_fields_device, dspmap_cost_paths_device) against what the parent
offers -- the plain static arrival fields of the same sources -- and against the route a user has without them: (d) copies of the cast
layer and the distance layer to the host, Dijkstra there, and an upload of the result.  The host Dijkstra is
scipy.sparse.csgraph.dijkstra on the directed grid graph (edge a -> b of weight w(b)) if scipy imports, else the numpy restatement of the
tests (tests/cost_ref.fields).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles /
voxel), each after 20 frames of the synthetic depth stream (scene.py); threshold 0.2, distance field at R = 20 voxels, cast grid inflated
by 0 and by 2 voxels, layer 0.

(a) the cost build for 1 / 16 / 64 fields (one source each, in free cells) at 0, 1 and 3 bands; (b) dspmap_build_reach_fields_device,
static, of the same sources, in the same interleaved run: at 0 bands the two compute the same fields (asserted), and the ratio at 1 and 3
bands is what the recurrence's "one reach step per occurring weight and level" predicts or not; (c) dspmap_cost_paths_device for 4 096
starts down the 16-field build at 3 bands, and the chain paths -> dspmap_shorten_paths_device -> dspmap_grow_boxes_device.  Device times
are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup` untimed ones, the arms interleaved
call by call; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs, and the tool asserts
that both routes give the same field.  It also reports what the feature is for: the mean and the minimum of the distance field along the
weighted paths against the unweighted paths from the same starts.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/cost_bench.py [--reps 200] [--warmup 20] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
DIST_R = 20
FIELDS = (1, 16, 64)
BANDS = {0: (), 1: ((0.45, 3),), 3: ((0.45, 3), (0.75, 2), (1.05, 1))}      # metres: 3, 5 and 7 voxels
N_START = 4096
MAX_LEN = 256
GROW = (8, 8, 8)


def host_field(cost_ref, cfg, w, src):
    """one field on the host: scipy's Dijkstra on the directed 6-neighbour graph of the free cells if scipy imports, else the restatement"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        return cost_ref.fields(cfg, w, src, 1)[0], "numpy restatement (tests/cost_ref.fields)"
    nz, ny, nx = w.shape
    idx = np.arange(w.size).reshape(w.shape)
    rows, cols, vals = [], [], []
    for a, b in ((np.s_[:, :, :-1], np.s_[:, :, 1:]), (np.s_[:, :-1, :], np.s_[:, 1:, :]), (np.s_[:-1, :, :], np.s_[1:, :, :])):
        for u, v in ((a, b), (b, a)):                                         # the step u -> v costs w(v)
            ok = (w[u] > 0) & (w[v] > 0)
            rows.append(idx[u][ok]); cols.append(idx[v][ok]); vals.append(w[v][ok].astype(np.float64))
    g = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(w.size, w.size)).tocsr()
    finite, inside, ijk = cost_ref.R.point_cells(cfg, src)
    s = int(idx[ijk[0, 2], ijk[0, 1], ijk[0, 0]])
    out = np.full(w.size, cost_ref.UNREACHED, np.uint16)
    if w.reshape(-1)[s] > 0:
        d = dijkstra(g, directed=True, indices=s)
        ok = d <= cost_ref.MAX_COST
        out[ok] = d[ok].astype(np.uint16)
    return out.reshape(w.shape), "scipy.sparse.csgraph.dijkstra"


def run(D, scene, name, args):
    from tests import cost_ref, reach_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)
    with torch.cuda.stream(st):
        m.build_distance_field(THRESHOLD, DIST_R)
        dist = m.distance_field(0)
        st.synchronize()

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    cfg = m.cfg
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "threshold": THRESHOLD, "distance_field_R": DIST_R, "bands_m_penalty": {str(k): [list(b) for b in v] for k, v in BANDS.items()}}
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    for r in (0, 2):
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, r)
            lay = reach_ref.unpack(m.cast_grid(0), w["nx"])
        cand = np.argwhere(~lay)
        assert len(cand) >= 64, "no room for 64 sources"
        pick = cand[rng.choice(len(cand), 64, replace=False)]
        src = reach_ref.points([tuple((-half + w["res"] * (c[::-1] + 0.5)).tolist()) + (k,) for k, c in enumerate(pick)])
        dsrc = torch.from_numpy(src.view(np.int32).reshape(-1, 4).copy()).cuda()
        starts = np.zeros(N_START, reach_ref.POINT_DTYPE)
        p = rng.uniform(-0.98, 0.98, (N_START, 3)) * half
        starts["x"], starts["y"], starts["z"], starts["field"] = p[:, 0], p[:, 1], p[:, 2], rng.integers(0, 16, N_START)
        dstarts = torch.from_numpy(starts.view(np.int32).reshape(-1, 4).copy()).cuda()
        torch.cuda.synchronize()
        # (a) the cost build, (b) the plain static reach build of the same sources, interleaved
        arms, keys = [], []
        for nf in FIELDS:
            arms.append(lambda nf=nf: m.build_reach_fields(dsrc[:nf], nf, max_steps=D.capi.REACH_MAX_STEPS))
            keys.append("reach_build_us_median_min_inflate%d_fields%d_static" % (r, nf))
            for nb, bands in BANDS.items():
                arms.append(lambda nf=nf, bands=bands: m.build_cost_fields(dsrc[:nf], nf, bands=bands, max_cost=D.capi.REACH_MAX_STEPS if not bands else D.capi.COST_MAX_COST))
                keys.append("cost_build_us_median_min_inflate%d_fields%d_bands%d" % (r, nf, nb))
        for k, v in zip(keys, timed(arms, args.reps)):
            out[k] = v
        with torch.cuda.stream(st):                                           # at 0 bands the two builds are the same fields
            m.build_reach_fields(dsrc[:16], 16, max_steps=D.capi.REACH_MAX_STEPS)
            m.build_cost_fields(dsrc[:16], 16, max_cost=D.capi.REACH_MAX_STEPS)
            assert np.array_equal(m.reach_field(None, 16), m.cost_field(None, 16)), "cost fields without bands differ from the reach fields"
        # (c) paths down the 16-field build at 3 bands, and the chain paths -> shorten -> boxes
        with torch.cuda.stream(st):
            m.build_cost_fields(dsrc[:16], 16, bands=BANDS[3])
            weights = m.cost_weights()
        out["weights_occurring_inflate%d" % r] = np.unique(weights).tolist()

        def chain():
            cost, cells = m.cost_paths(dstarts, MAX_LEN)
            info, seg, end = m.shorten_paths(cost, cells, window=64, max_seg=32)
            return m.grow_boxes(seg.view(-1, 8), GROW)

        pm, cm = timed([lambda: m.cost_paths(dstarts, MAX_LEN), chain], args.reps)
        out["cost_paths_us_median_min_inflate%d_%d_starts_max_len_%d" % (r, N_START, MAX_LEN)] = pm
        out["chain_paths_shorten_boxes_us_median_min_inflate%d_%d_starts" % (r, N_START)] = cm
        # what the weights are for: the clearance along the weighted paths against the unweighted paths from the same starts
        with torch.cuda.stream(st):
            wc, wcells = (x.cpu().numpy() for x in m.cost_paths(dstarts, MAX_LEN))
            m.build_cost_fields(dsrc[:16], 16)
            pc, pcells = (x.cpu().numpy() for x in m.cost_paths(dstarts, MAX_LEN))
        both = (wc >= 0) & (pc >= 0) & (wcells[:, -1] < 0) & (pcells[:, -1] < 0)                         # complete in both builds
        flat = dist.reshape(-1)
        for tag, cells in (("weighted", wcells[both]), ("unweighted", pcells[both])):
            on = flat[cells[cells >= 0]]
            out["clearance_m_mean_min_cells_along_%s_paths_inflate%d" % (tag, r)] = [round(float(on.mean()), 4), round(float(on.min()), 4), int(on.size)]
        out["paths_complete_in_both_inflate%d" % r] = int(both.sum())
        # (d) the route without the feature, one field: the two layers to the host, Dijkstra there, the field back to the device
        for nb in (0, 3):
            tcopy, tdij, tup = [], [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                grid, dl = m.cast_grid(0), m.distance_field(0)
                t1 = time.perf_counter()
                hw = cost_ref.weights(reach_ref.unpack(grid, w["nx"]), dl, BANDS[nb])
                want, how = host_field(cost_ref, cfg, hw, src[:1])
                t2 = time.perf_counter()
                torch.from_numpy(want.astype(np.int32)).cuda()
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                tcopy.append((t1 - t0) * 1e3); tdij.append((t2 - t1) * 1e3); tup.append((t3 - t2) * 1e3)
            out["host_ms_copies_dijkstra_upload_inflate%d_bands%d_fields1" % (r, nb)] = [round(float(np.median(x)), 3) for x in (tcopy, tdij, tup)]
            out["host_dijkstra"] = how
            with torch.cuda.stream(st):
                m.build_cost_fields(src[:1], 1, bands=BANDS[nb])
                got = m.cost_field(0)
            assert np.array_equal(got, want), "the device and the host route disagree"
            out["reached_fraction_inflate%d_bands%d" % (r, nb)] = round(float((got != cost_ref.UNREACHED).mean()), 4)
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
