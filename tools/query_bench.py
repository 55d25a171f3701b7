"""Timing of the point / trajectory queries (dspmap_query_occupancy_device, dspmap_trajectory_risk_device) against the whole-grid
readouts a planner would use otherwise, on config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) after 20 frames of the synthetic
depth stream (scene.py: walls, boxes and walking pedestrians).  HIP events on the handle's stream (a torch stream) around `--reps`
back-to-back calls after `--warmup` untimed ones; the host readout (getFutureStatus: combine + 4.2 MB copy + synchronisation) is
timed on the wall clock.  Prints one JSON line.  bench.py is not involved.

    python tools/query_bench.py [--reps 200] [--warmup 20]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness


def run(D, scene, name, args):
    w = harness.WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)   # (the frames clear the prediction before every frame but never after the last one:
    # the timed queries read its live prediction; a pending clear would make every t >= 0 sample read 0 without touching the accumulators)

    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]], np.float32) * np.float32(w["res"]) * np.float32(0.5)
    pred = np.array([0.05, 0.2, 0.5, 1.0, 1.5, 2.0], np.float32)

    def samples(n):
        q = np.empty((n, 4), np.float32)
        q[:, :3] = rng.uniform(-1, 1, (n, 3)) * half
        q[:, 3] = np.concatenate([[-1.0], pred])[rng.integers(0, 7, n)]
        return torch.from_numpy(q).cuda()

    def trajectories(k, s):
        start = rng.uniform(-0.8, 0.8, (k, 1, 3)) * half
        vel = rng.uniform(-1.5, 1.5, (k, 1, 3))
        ts = np.linspace(0.0, 2.0, s)[None, :, None]
        q = np.concatenate([start + vel * ts, np.broadcast_to(ts, (k, s, 1))], 2).astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(q)).cuda()

    def timed(fn):
        """mean device time (us) of one call, events on the handle's stream"""
        with torch.cuda.stream(st):
            for _ in range(args.warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(args.reps):
                fn()
            e1.record(st)
            e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / args.reps

    q = samples(131072)
    tr = trajectories(4096, 32)
    torch.cuda.synchronize()
    # the prediction is live: t >= 0 samples read non-zero future status (and keep reading the same after the timed calls)
    live = q[q[:, 3] >= 0].contiguous()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        probe = m.query_occupancy(live, radius=0.3, outside=0.0)
        st.synchronize()
    assert int((probe > 0).sum()) > 1000, "the future accumulators read as cleared: the timings would skip their gathers"
    out = {}
    for r in (0.0, 0.15, 0.3):
        out["query_131072_r%.2f_us" % r] = round(timed(lambda: m.query_occupancy(q, radius=r)), 2)
    out["risk_4096x32_r0.30_us"] = round(timed(lambda: m.trajectory_risk(tr, radius=0.3)), 2)
    with torch.cuda.stream(st):
        assert torch.equal(m.query_occupancy(live, radius=0.3, outside=0.0), probe)
        st.synchronize()
    out["live_future_samples"] = int((probe > 0).sum())
    out["future_device_combine_us"] = round(timed(lambda: m.L.dspmap_future_device(m.h)), 2)
    fut = np.zeros((m.V_local, m.T), np.float32)
    for _ in range(5):
        m.L.dspmap_get_future(m.h, fut.ctypes.data_as(D.capi.C.c_void_p))
    t0 = time.perf_counter()
    n_host = 50
    for _ in range(n_host):
        m._chk(m.L.dspmap_get_future(m.h, fut.ctypes.data_as(D.capi.C.c_void_p)))
    out["get_future_status_host_us"] = round((time.perf_counter() - t0) * 1e6 / n_host, 2)
    out["grid_bytes"] = int(fut.nbytes)
    out["config"] = "B: 66x66x40 @ 0.15 m, 24 particles/voxel, %d frames of scene.py; %d timed calls after %d" % (args.frames, args.reps, args.warmup)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    harness.main(run, harness.parser(reps=200, warmup=20, frames=20, only=False), names=("B",))


if __name__ == "__main__":
    main()
