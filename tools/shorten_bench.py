"""Timing of the shortened paths (dspmap_shorten_paths_device) against the route a user has without them: copies of cells_out and of the
cast grid to the host and the string-pull there.  The host string-pull is the numpy restatement of the tests (tests/shorten_ref.shorten on
tests/cast_ref.cast): every greedy round one cast call vectorised over all paths x candidates, not per-path Python loops.  Workloads:
config B (66 x 66 x 40 @ 0.15 m, 24 particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic
depth stream (scene.py); L = 7 layers, threshold 0.2, grids inflated by 0 and by 2 voxels.  The paths are the timeline paths of 4 096
starts through the scheduled 16-field build (t_start = 0, step_seconds = voxel / 1.5 m/s, max_steps 256: rows of 257 cells), shortened
with the build's schedule, max_seg 32 (8 in the chain, where the window is 64; paths that would need more are counted).  Entries behind a
path's segments are the all-zero padding, which grow_boxes takes as seeds at the map centre: the chain pays for them as a caller who does
not compact would.

(a) the device time of dspmap_shorten_paths_device at the windows 8 and 64; (b) the chain timeline paths -> shorten -> grow_boxes
(max_grow 8, 8, 4) on device tensors with no host read, and its three calls alone; (c) the route without the feature at both windows: the
cells_out and cast_grid() copies, then the restatement -- with the assertion that both routes give the same records, bit for bit.  Device
times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls after `--warmup` untimed ones, the arms
interleaved call by call; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs.
Prints one JSON line per workload.  bench.py is not involved.

    python tools/shorten_bench.py [--reps 200] [--warmup 20] [--host-reps 1] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
SPEED = 1.5          # m/s: a scheduled front crosses one voxel per step_seconds = res / SPEED
N_FIELDS = 16
N_START = 4096
MAX_STEPS = 256
MAX_SEG = 32
CHAIN_MAX_SEG = 8   # what the chain asks for at window 64 (a caller sizes max_seg to the window); paths that need more are counted
WINDOWS = (8, 64)
GROW = (8, 8, 4)


def run(D, scene, name, args):
    from tests import reach_ref, shorten_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    cfg = m.cfg
    step = w["res"] / SPEED
    sched = dict(t_start=0.0, step_seconds=step)
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": m.T + 1, "threshold": THRESHOLD, "scheduled_step_seconds": round(step, 4), "paths": N_START, "max_len": MAX_STEPS + 1,
           "max_seg": MAX_SEG, "chain_max_seg": CHAIN_MAX_SEG, "max_grow": list(GROW)}
    rng = np.random.default_rng(0)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    for r in (0, 2):
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, r)
            lay = reach_ref.unpack(m.cast_grid(), w["nx"])
        cand = np.argwhere(~lay.any(0))
        assert len(cand) >= N_FIELDS, "no room for the sources"
        pick = cand[rng.choice(len(cand), N_FIELDS, replace=False)]
        src = reach_ref.points([tuple((-half + w["res"] * (c[::-1] + 0.5)).tolist()) + (k,) for k, c in enumerate(pick)])
        dsrc = torch.from_numpy(src.view(np.int32).reshape(-1, 4).copy()).cuda()
        starts = np.zeros(N_START, reach_ref.POINT_DTYPE)
        p = rng.uniform(-0.98, 0.98, (N_START, 3)) * half
        starts["x"], starts["y"], starts["z"], starts["field"] = p[:, 0], p[:, 1], p[:, 2], rng.integers(0, N_FIELDS, N_START)
        dstarts = torch.from_numpy(starts.view(np.int32).reshape(-1, 4).copy()).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            m.build_reach_timeline(dsrc, N_FIELDS, max_steps=MAX_STEPS, **sched)
            dsteps, dcells = m.reach_timeline_paths(dstarts, MAX_STEPS + 1)
            dinfo, dseg, _ = m.shorten_paths(dsteps, dcells, window=64, max_seg=CHAIN_MAX_SEG, **sched)
            st.synchronize()
        out["chain_truncated_paths_inflate%d" % r] = int(dinfo[:, 3].sum())
        tag = "inflate%d" % r

        def shorten(window):
            return m.shorten_paths(dsteps, dcells, window=window, max_seg=MAX_SEG, **sched)

        def chain():
            s, c = m.reach_timeline_paths(dstarts, MAX_STEPS + 1)
            seg = m.shorten_paths(s, c, window=64, max_seg=CHAIN_MAX_SEG, **sched)[1]
            return m.grow_boxes(seg.view(-1, 8), GROW)

        # (a), (b): every arm in one interleaved run
        arms = [lambda: shorten(8), lambda: shorten(64), lambda: m.reach_timeline_paths(dstarts, MAX_STEPS + 1),
                lambda: m.grow_boxes(dseg.view(-1, 8), GROW), chain]
        keys = ["shorten_window8", "shorten_window64", "timeline_paths", "grow_boxes_%d_seeds" % (N_START * CHAIN_MAX_SEG), "chain_paths_shorten_window64_boxes"]
        for k, v in zip(keys, timed(arms, args.reps)):
            out["us_median_min_%s_%s" % (tag, k)] = v
        # (c) the route without the feature, and the same records from both
        for window in WINDOWS:
            with torch.cuda.stream(st):
                info, seg, end = shorten(window)
                st.synchronize()
            info, seg, end = shorten_ref.info_of(info.cpu().numpy()), seg.cpu().numpy(), end.cpu().numpy()
            tc, th = [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                hsteps, hcells = dsteps.cpu().numpy(), dcells.cpu().numpy()
                grid = m.cast_grid()
                t1 = time.perf_counter()
                want = shorten_ref.shorten(cfg, reach_ref.unpack(grid, w["nx"]), hsteps, hcells, window=window, max_seg=MAX_SEG, **sched)
                t2 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                th.append((t2 - t1) * 1e3)
            assert np.array_equal(info, want[0]) and np.array_equal(end, want[2]), "the device and the host route disagree"
            assert np.array_equal(seg.view(np.uint32), want[1].view(np.uint32)), "the device and the host route disagree on the records"
            out["host_ms_copies_restatement_%s_window%d" % (tag, window)] = [round(float(np.median(tc)), 3), round(float(np.median(th)), 1)]
            has = info["n_cells"] > 1
            out["paths_with_segments_mean_cells_mean_segments_blocked_truncated_%s_window%d" % (tag, window)] = [
                int(has.sum()), round(float(info["n_cells"][has].mean()), 1) if has.any() else None,
                round(float(info["n_segments"][has].mean()), 2) if has.any() else None, int(info["n_blocked"].sum()), int(info["truncated"].sum())]
    out["host_string_pull"] = "numpy restatement (tests/shorten_ref.shorten)"
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20, host_reps=1)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
