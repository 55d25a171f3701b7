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
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

N_TIMES = (1, 6, 16, 64)
N_QUERY = 131072
HOST_TIMES = 6
FLOAT_ATOMIC_TBS = 1.3


def times_of(n):
    return (np.arange(n, dtype=np.float32) * np.float32(3.0 / max(n - 1, 1))).astype(np.float32) if n > 1 else np.array([0.5], np.float32)


def run(D, scene, name, state, args):
    from tests import forecast_ref
    w = WORKLOADS[name]
    fed = 0 if state == "moving" else args.frames
    m, st = harness.open_map(D, scene, name, fed, spare=args.frames + 8 - fed)
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"])}
    if state == "moving":
        with torch.cuda.stream(st):
            m.seed_uniform(m.slots, 0.01, 99, vmax=1.0)
            st.synchronize()
        out["state"] = "seed_uniform_moving: %d particles per voxel, |v| <= 1 m/s" % m.slots
    else:
        out["state"] = "%d frames of scene.py" % args.frames

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

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
            for pts, pos, quat, t in m.scene_frames[args.frames:]:
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
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=1)
    ap.add_argument("--state", choices=("stream", "moving"), default=None)

    def states(D, scene, name, args):
        for state in ([args.state] if args.state else ["stream", "moving"]):
            run(D, scene, name, state, args)

    harness.main(states, ap)


if __name__ == "__main__":
    main()
