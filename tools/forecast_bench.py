"""Timing of the occupancy forecast at caller-chosen times (dspmap_build_forecast, dspmap_query_forecast_device) against the route a user
has without it: (c) export_state() -- 32 B per particle over the bus -- and the rollout on the host (the numpy restatement of the tests,
tests/forecast_ref.layers: whole-array operations per layer, not per-particle Python loops).  Workloads: config B (66 x 66 x 40 @ 0.15 m,
24 particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each (i) after 20 frames of the synthetic depth stream (scene.py): the
mostly-static map the design aims at, and (ii) after seed_uniform_moving with every slot filled and every particle moving: the
atomic-bound worst case.

(a) the build at 1 / 6 / 16 / 64 times; (b) the query for 131 072 samples with and without DSPMAP_FORECAST_LERP; (d) for context, stage 7
(resample + rollout) of dspmap_get_stage_ms over frames of the same stream on the same map; (e) for the all-moving arms the bytes the
64-bit integer atomics add (particles x layers x 8 B, destinations outside the map included: an upper bound) divided by the build's time,
next to the ~1.3 TB/s the float atomics of this chip reach.  Device times are HIP events on the handle's stream (a torch stream) around
EVERY one of `--reps` calls after `--warmup` untimed ones, the arms interleaved call by call; the median is reported (and the minimum).
The host route is wall time, the median of `--host-reps` runs, and the tool asserts that both routes give the same layers.  Prints one
JSON line per workload and state.  bench.py is not involved.

    python tools/forecast_bench.py [--reps 200] [--warmup 3] [--host-reps 1] [--only B|L] [--state stream|moving]
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
N_TIMES = (1, 6, 16, 64)
N_QUERY = 131072
HOST_TIMES = 6
FLOAT_ATOMIC_TBS = 1.3


def times_of(n):
    return (np.arange(n, dtype=np.float32) * np.float32(3.0 / max(n - 1, 1))).astype(np.float32) if n > 1 else np.array([0.5], np.float32)


def run(D, scene, name, state, args):
    from tests import forecast_ref
    w = WORKLOADS[name]
    m = D.DSPMap(D.make_config(seed=1234, **w))
    m._chk(m.L.dspmap_init_device(m.h))
    sc = scene.CorridorScene(w["nx"] * w["res"], w["ny"] * w["res"], w["nz"] * w["res"], seed=1234, device="cuda")
    torch.use_deterministic_algorithms(True)
    frames = [sc.frame(f / 30.0) + (f / 30.0,) for f in range(args.frames + 8)]
    torch.use_deterministic_algorithms(False)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    m._chk(m.L.dspmap_set_stream(m.h, st.cuda_stream))
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"])}
    with torch.cuda.stream(st):
        if state == "moving":
            m.seed_uniform(m.slots, 0.01, 99, vmax=1.0)
            out["state"] = "seed_uniform_moving: %d particles per voxel, |v| <= 1 m/s" % m.slots
        else:
            for f, (pts, pos, quat, t) in enumerate(frames[:args.frames]):
                if f:
                    m.clearOccupancyMapPrediction()
                assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            out["state"] = "%d frames of scene.py" % args.frames
        st.synchronize()

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

    cfg = m.cfg
    # (c) the host route first (it also counts the particles): the state copy, then the rollout on the CPU -- and the same answer
    tc, tg = [], []
    ht = times_of(HOST_TIMES)
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        voxel, slot, rec = m.export_state()
        t1 = time.perf_counter()
        want, acc, dropped = forecast_ref.layers(cfg, voxel, rec, ht)
        t2 = time.perf_counter()
        tc.append((t1 - t0) * 1e3)
        tg.append((t2 - t1) * 1e3)
    with torch.cuda.stream(st):
        m.build_forecast(ht)
        got = m.forecast()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the device and the host route disagree"
    n_part = len(voxel)
    n_mov = int(((rec[:, 1] != 0) | (rec[:, 2] != 0)).sum())
    out["particles_moving"] = [n_part, n_mov]
    out["host_ms_export_rollout_%d_times" % HOST_TIMES] = [round(float(np.median(tc)), 1), round(float(np.median(tg)), 1)]
    del voxel, slot, rec, want, acc, got
    # (a) the build
    arms = [lambda t=times_of(n): m.build_forecast(t) for n in N_TIMES]
    for n, v in zip(N_TIMES, timed(arms, args.reps)):
        out["build_us_median_min_%d_times" % n] = v
        if state == "moving":   # (e)
            out["atomic_TBs_%d_times" % n] = round(n_mov * n * 8 / (v[0] * 1e-6) / 1e12, 3)
    if state == "moving":
        out["float_atomic_TBs_of_the_guide"] = FLOAT_ATOMIC_TBS
    # (b) the query
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    q = np.concatenate([rng.uniform(-1.0, 1.0, (N_QUERY, 3)) * half, rng.uniform(-0.1, 3.2, (N_QUERY, 1))], 1).astype(np.float32)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        m.build_forecast(times_of(16))
    qa, qb = timed([lambda: m.query_forecast(dq), lambda: m.query_forecast(dq, lerp=True)], args.reps)
    out["query_us_median_min_%d_samples" % N_QUERY] = qa
    out["query_lerp_us_median_min_%d_samples" % N_QUERY] = qb
    # (d) the frame's own resample + rollout on the same map (stage 7), over frames of the same stream
    if state == "stream":
        with torch.cuda.stream(st):
            m.set_profiling(True)
            for pts, pos, quat, t in frames[args.frames:]:
                m.clearOccupancyMapPrediction()
                assert m.update_device(pts.data_ptr(), pts.shape[0], pos, t, quat) == 1
            st.synchronize()
            ms, nf = m.stage_ms()
            m.set_profiling(False)
        out["frame_stage7_resample_us_per_frame"] = round(ms["resample"] / max(nf, 1) * 1000.0, 1) if nf else None
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--state", choices=("stream", "moving"), default=None)
    args = ap.parse_args()
    import build_ext
    build_ext.build()
    import dsp_map_amd as D
    scene = importlib.import_module("dsp-map_amd.scene")
    for name in ([args.only] if args.only else ["B", "L"]):
        for state in ([args.state] if args.state else ["stream", "moving"]):
            run(D, scene, name, state, args)


if __name__ == "__main__":
    main()
