"""Timing of the free boxes grown in the cast grid (dspmap_grow_boxes_device) against the route a user has without them: (h) a cast_grid()
copy of all layers to the host and a growth loop there over the same seeds.  The host loop is the numpy restatement of the tests
(tests/corridor_ref.grow) on the WHOLE batch: the grid's words unpacked to bool cells, one summed volume (three cumulative sums) per
distinct set of tested layers, then the rounds and faces of the definition with every face test one vectorised expression over the
seeds -- a batched loop, not a per-box Python loop, which would be slower still.  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24
particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py); L = 7 layers,
threshold 0.2, grids inflated by 0 and by 2 voxels.

32 768 seeds of 0.3 .. 1.5 m with both ends inside the map, static (ta < 0) and space-time (ta = 0, tb = |ab| / 1.5 m/s), grown at
max_grow (8, 8, 4) and (64, 64, 64).  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps`
calls after `--warmup` untimed ones, the arms interleaved call by call; the median is reported (and the minimum).  The host route is
wall time, the median of `--host-reps` runs.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/corridor_bench.py [--reps 200] [--warmup 20] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

THRESHOLD = 0.2
N_SEED = 32768
SPEED = 1.5      # m/s along a space-time seed
GROWS = ((8, 8, 4), (64, 64, 64))


def seeds(w, n, seed=0):
    """[n, 8] float32, both ends inside the map, 0.3 .. 1.5 m long (a random direction, redrawn until b is inside)"""
    rng = np.random.default_rng(seed)
    half = np.array([w["nx"], w["ny"], w["nz"]], np.float64) * w["res"] * 0.5
    a = rng.uniform(-0.98, 0.98, (n, 3)) * half
    b = np.empty_like(a)
    todo = np.arange(n)
    while todo.size:
        d = rng.standard_normal((todo.size, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cand = a[todo] + d * rng.uniform(0.3, 1.5, (todo.size, 1))
        ok = (np.abs(cand) < 0.98 * half).all(1)
        b[todo[ok]] = cand[ok]
        todo = todo[~ok]
    seg = np.zeros((n, 8), np.float32)
    seg[:, 0:3], seg[:, 4:7] = a, b
    return seg, np.linalg.norm(b - a, axis=1)


def run(D, scene, name, args):
    from tests import corridor_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames)

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    seg, length = seeds(w, N_SEED)
    seg_static, seg_time = seg.copy(), seg.copy()
    seg_static[:, 3] = seg_static[:, 7] = -1.0
    seg_time[:, 7] = (length / SPEED).astype(np.float32)
    ds, dt = torch.from_numpy(seg_static).cuda(), torch.from_numpy(seg_time).cuda()
    torch.cuda.synchronize()
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel, %d frames of scene.py" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"], args.frames),
           "layers": m.T + 1, "threshold": THRESHOLD, "seeds": N_SEED, "mean_length_m": round(float(length.mean()), 2),
           "host_loop": "numpy restatement (tests/corridor_ref.grow) on all %d seeds: summed volumes per set of tested layers, vectorised face tests" % N_SEED}
    for r in (0, 2):
        with torch.cuda.stream(st):
            m.build_cast_grid(THRESHOLD, r)
            st.synchronize()
        arms, keys = [], []
        for g in GROWS:
            for tag, d in (("static", ds), ("spacetime", dt)):
                arms.append(lambda g=g, d=d: m.grow_boxes(d, g))
                keys.append("inflate%d_grow_%d_%d_%d_%s" % ((r,) + g + (tag,)))
        for k, v in zip(keys, timed(arms, args.reps)):
            out["device_us_median_min_" + k] = v
        with torch.cuda.stream(st):
            boxes = m.grow_boxes(dt, GROWS[0])
            st.synchronize()
        ok = boxes["status"] == 0
        ext = (boxes["hi"] - boxes["lo"] + 1)[ok].float()
        out["inflate%d_ok_fraction_mean_extent_8_8_4_spacetime" % r] = [round(float(ok.float().mean()), 4)] + [round(float(v), 1) for v in ext.mean(0)]
        # (h) the host route: the grid copy, then the growth on the CPU over the same seeds
        for g in GROWS:
            tc, tg = [], []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                grid = m.cast_grid()
                t1 = time.perf_counter()
                want = corridor_ref.grow(m.cfg, corridor_ref.unpack(grid, w["nx"]), seg_time, g)
                t2 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                tg.append((t2 - t1) * 1e3)
            out["host_ms_copy_growth_inflate%d_grow_%d_%d_%d_spacetime" % ((r,) + g)] = [round(float(np.median(tc)), 3), round(float(np.median(tg)), 1)]
            with torch.cuda.stream(st):
                got = m.grow_boxes(seg_time, g)
            assert got.tobytes() == want.tobytes(), "the device and the host route disagree"
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=20, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
