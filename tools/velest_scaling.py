#!/usr/bin/env python3
"""What the device velocity estimator's matching costs a frame as the number of clusters grows.

For K = 32, 64, 65, 128, 300 clusters, one fresh process per K and in ascending order, two scenes of tests/velest_scenes.py are run as
device-resident frames with DSPMAP_P_ESTIMATOR_QUEUE = 0 (the estimator is a forked branch of the frame: it sits on the frame's
critical path as soon as it is the longer branch):
  all_gated(K)  every pair of a new and an old cluster is gated: an all-equal cost matrix, N (N + 1) / 2 steps of the Hungarian
  benign(K)     the same K sticks moved by a few centimetres: N .. 2 N steps
and reported is  median frame time with estimator mode 2  -  median frame time of the same frames with mode 0  (host clock around
update_device + synchronise; the two handles alternate call by call; warm-up frames first).

The worst case is then fitted as  time = a * steps * ceil((N + 1) / 64)  over the sizes with N > 64, and the fit is extended to the
estimator's capacity of 1 228 clusters.  --capacity runs that size ONLY if the fit predicts less than one second for it.

    python tools/velest_scaling.py [--sizes 32,64,65,128,300] [--out table.json] [--capacity]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dsp-map_amd"))


def scene_for(kind, K):
    from tests import velest_scenes as vs
    if kind == "all_gated":
        return vs.all_gated(K)
    return vs.benign([K, K], "benign_%d" % K, rows=12 if K <= 200 else 21)


def matching_steps(sc):
    """(N, steps) of the matching of frame 1 against frame 0, counted on the oracle's algorithm"""
    import numpy as np
    from oracle import oracle_py as orc
    from tests import velest_scenes as vs
    feats = []
    for pts in sc.frames[:2]:
        w = vs.world(pts)
        ng = w[w[:, 2] > vs.RES_F]
        label, K = orc.euclidean_clusters(ng, float(vs.TOL))
        f = np.array([[*np.cumsum(ng[label == c], axis=0, dtype=np.float32)[-1] / np.float32((label == c).sum()), (label == c).sum()]
                      for c in range(K)], np.float32)
        feats.append(f[(f[:, 3] <= 200) & (f[:, 2] <= 1.5)])
    cost, _ = vs.cost_matrix(feats[1], feats[0])
    return max(cost.shape), vs.hungarian_steps(cost)[1]


def child(kind, K):
    import torch
    import dsp_map_amd as dsp
    from tests import common
    from tests import velest_scenes as vs
    sc = scene_for(kind, K)
    N, steps = matching_steps(sc)
    clouds = [torch.from_numpy(p).cuda() for p in sc.frames[:2]]
    maps = {}
    for mode in (2, 0):
        m = dsp.DSPMap(dsp.make_config(**vs.CFG))
        m.set_tables(*common.tables(1))
        m.set_param(dsp.capi.P_VELOCITY_ESTIMATOR, mode)
        m.set_param(dsp.capi.P_ESTIMATOR_QUEUE, 0)
        maps[mode] = m
    times = {2: [], 0: []}

    def frame(f, record):
        slow = 0.0
        for mode, m in maps.items():
            t0 = time.perf_counter()
            rc = m.update_device(clouds[f % 2].data_ptr(), len(sc.frames[f % 2]), sc.pos, f * sc.dt, sc.quat)
            m.sync()
            dt = time.perf_counter() - t0
            assert rc == 1
            slow = max(slow, dt)
            if record:
                times[mode].append(dt)
        return slow

    frame(0, False)                                  # (no matching yet: nothing to match against)
    probe = frame(1, False)
    f = 2
    for _ in range(0 if probe > 1.0 else 4):         # warm-up; a frame that takes seconds has nothing left to warm up
        frame(f, False); f += 1
    reps = 60 if probe < 0.02 else (20 if probe < 0.2 else (6 if probe < 1.0 else 3))
    for _ in range(reps):
        frame(f, True); f += 1
    assert maps[2].L.dspmap_debug_estimator_path(maps[2].h) == 3
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps(dict(kind=kind, K=K, N=N, steps=steps, frames=reps, ms_mode2=1e3 * med[2], ms_mode0=1e3 * med[0],
                          ms_estimator=1e3 * (med[2] - med[0]), ms_mode2_min=1e3 * min(times[2]), ms_mode2_max=1e3 * max(times[2]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64,65,128,300")
    ap.add_argument("--out")
    ap.add_argument("--capacity", action="store_true", help="also run all_gated(1228) if the fit predicts less than one second")
    ap.add_argument("--limit", type=int, default=150, help="seconds per child process")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]))
    rows = []

    def run(kind, K):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", kind, str(K)],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print("stopping: %s(%d) ended with status %d" % (kind, K, r.returncode), flush=True)
            return False
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
        return True

    work = lambda N: (N * (N + 1) // 2) * (-(-(N + 1) // 64))
    ok = True
    for K in sorted(int(x) for x in a.sizes.split(",")):
        worst = [r for r in rows if r["kind"] == "all_gated"]
        ok = run("benign", K)
        if ok and worst and worst[-1]["ms_estimator"] * work(K) / work(worst[-1]["N"]) > 5000.0:
            print("all_gated(%d) not run: all_gated(%d) predicts more than 5 s per frame" % (K, worst[-1]["N"]), flush=True)
            continue
        ok = ok and run("all_gated", K)
        if not ok:
            break
    fit = [r for r in rows if r["kind"] == "all_gated" and r["N"] > 64]
    summary = dict(rows=rows)
    if fit:
        coef = sum(r["ms_estimator"] * work(r["N"]) for r in fit) / sum(work(r["N"]) ** 2 for r in fit)     # least squares through 0
        summary["fit_ms_per_step_visit"] = coef
        summary["predicted_ms"] = {N: coef * work(N) for N in (128, 300, 512, 1228)}
        print(json.dumps({k: summary[k] for k in ("fit_ms_per_step_visit", "predicted_ms")}), flush=True)
        if a.capacity and ok:
            if summary["predicted_ms"][1228] < 1000.0:
                run("all_gated", 1228)
            else:
                print("all_gated(1228) not run: the fit predicts %.1f s" % (summary["predicted_ms"][1228] / 1e3), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
