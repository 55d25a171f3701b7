"""Timing of the known-space layer (dspmap_known_integrate, dspmap_mask_cast_grid, dspmap_query_known_device) against the route a user has
without it: dspmap_get_observations plus dspmap_get_view -- the frame's observations, rotated planes and farthest returns copied to the
host -- and the classification of every cell on the CPU (the numpy restatement of the tests, tests/known_ref.classify: whole-array
operations, no per-cell Python loop).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles /
voxel), each after 20 frames of the synthetic depth stream (scene.py).

Arms, interleaved call by call: (m) dspmap_known_reset, which is one hipMemsetAsync of the stamp buffer -- the yardstick for a kernel that
writes at most 4 B per cell; (a) dspmap_known_integrate; (b) dspmap_mask_cast_grid on a grid built once; (c) 131 072 samples through
dspmap_query_known_device.  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after
`--warmup` untimed ones; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs, and
the tool asserts that both routes stamp the same cells.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/known_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dsp-map_amd"))

WORKLOADS = {"B": dict(nx=66, ny=66, nz=40, res=0.15, ppv=24), "L": dict(nx=132, ny=132, nz=60, res=0.15, ppv=9)}
N_QUERY = 131072


def run(D, scene, name, args):
    from tests import known_ref
    w = WORKLOADS[name]
    m = D.DSPMap(D.make_config(seed=1234, **w))
    m._chk(m.L.dspmap_init_device(m.h))
    sc = scene.CorridorScene(w["nx"] * w["res"], w["ny"] * w["res"], w["nz"] * w["res"], seed=1234, device="cuda")
    torch.use_deterministic_algorithms(True)
    frames = [sc.frame(f / 30.0) + (f / 30.0,) for f in range(args.frames)]
    torch.use_deterministic_algorithms(False)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
           "state": "%d frames of scene.py" % args.frames, "stamp_bytes": 4 * m.V}
    with torch.cuda.stream(st):
        for f, (pts, pos, quat, t) in enumerate(frames):
            if f:
                m.clearOccupancyMapPrediction()
            assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
        st.synchronize()
    cur = np.array(frames[-1][1], np.float32)
    counter = int(m.get_param(D.capi.P_UPDATE_COUNTER))
    margin = float(m.get_param(D.capi.P_OCCLUSION_MARGIN))

    def timed(fns, reps):
        """device time (us) of each of reps calls of every arm, the arms interleaved call by call -> [(median, min)] per arm"""
        with torch.cuda.stream(st):
            for _ in range(args.warmup):
                for fn in fns:
                    fn()
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
            for row in ev:
                for fn, (e0, e1) in zip(fns, row):
                    e0.record(st)
                    fn()
                    e1.record(st)
            st.synchronize()
        t = np.array([[e0.elapsed_time(e1) * 1000.0 for e0, e1 in row] for row in ev])
        return [(round(float(np.median(t[:, j])), 2), round(float(t[:, j].min()), 2)) for j in range(len(fns))]

    # the route without the feature: the frame's observations and view over the bus, every cell classified on the CPU
    tc, tg = [], []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        m.observations()
        ph, pv, ml = m.view()
        t1 = time.perf_counter()
        seen = known_ref.classify(m.cfg, cur, ph, pv, ml, margin)[0]
        t2 = time.perf_counter()
        tc.append((t1 - t0) * 1e3)
        tg.append((t2 - t1) * 1e3)
    with torch.cuda.stream(st):
        m.reset_known()
        m.integrate_known()
        ages = m.known_age()
        m.build_cast_grid(0.2, 1)
    assert np.array_equal(ages == 0, seen) and np.array_equal(ages == -1, ~seen), "the device and the host route disagree"
    out["cells_seen_of"] = [int(seen.sum()), int(seen.size)]
    out["host_ms_copies_classification"] = [round(float(np.median(tc)), 2), round(float(np.median(tg)), 1)]
    out["frame_counter"] = counter
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    q = np.concatenate([rng.uniform(-1.0, 1.0, (N_QUERY, 3)) * half, np.zeros((N_QUERY, 1))], 1).astype(np.float32)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    arms = [m.reset_known, m.integrate_known, lambda: m.mask_cast_grid(0), lambda: m.query_known(dq)]
    keys = ["memset_stamps_us_median_min", "integrate_us_median_min", "mask_%d_layers_us_median_min" % (m.T + 1), "query_us_median_min_%d_samples" % N_QUERY]
    for k, v in zip(keys, timed(arms, args.reps)):
        out[k] = v
    out["integrate_GBs_of_stamp_bytes"] = round(4 * m.V / (out[keys[1]][0] * 1e-6) / 1e9, 1)
    with torch.cuda.stream(st):
        again = m.known_age()
    assert np.array_equal(again, ages), "the timed calls changed the layer"
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    args = ap.parse_args()
    import build_ext
    build_ext.build()
    import dsp_map_amd as D
    scene = importlib.import_module("dsp-map_amd.scene")
    for name in ([args.only] if args.only else ["B", "L"]):
        run(D, scene, name, args)


if __name__ == "__main__":
    main()
