"""Timing of the frontier extension (dspmap_build_frontiers) against the route a user has without it: dspmap_get_known (4 B per voxel) and
dspmap_get_cast_grid copied to the host, then the six-neighbour stencil, the cell list and the block sums on the CPU (the numpy restatement
of the tests, tests/frontier_ref: whole-array operations, no per-cell Python loop).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24
particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py) with the
known-space layer integrated after every frame and a cast grid built from the last one.

Arms, interleaved call by call: dspmap_build_frontiers with block 1, 4 and 16 (one memset of the blocks' accumulators and four launches
each), first with the block sums merged per wave and block (the default), then with one set of atomics per frontier cell
(DSPMAP_P_FRONTIER_MERGE = 0).  Device times are HIP events on the handle's stream (a torch stream) around EVERY one of `--reps` calls
after `--warmup` untimed ones; the median is reported (and the minimum).  The host route is wall time, the median of `--host-reps` runs, and the tool asserts that
both routes give the same cells and the same blocks for every block size.  It ends with one pass of the whole loop: the block centres as
candidate views through dspmap_score_views.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/frontier_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

BLOCKS = (1, 4, 16)
MAX_AGE, MIN_UNKNOWN = 10, 1


def unpack(words, nx):
    """uint64 [nz, ny, W] -> bool [nz, ny, nx]"""
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[:-1] + (-1,))[..., :nx].astype(bool)


def run(D, scene, name, args):
    from tests import frontier_ref as R
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames, after_frame=lambda m: m.integrate_known())
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
           "state": "%d frames of scene.py, integrate_known after each, build_cast_grid(0.2, 1)" % args.frames,
           "max_age_min_unknown": [MAX_AGE, MIN_UNKNOWN]}
    with torch.cuda.stream(st):
        m.build_cast_grid(0.2, 1)
        st.synchronize()

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    # the route without the feature: ages and grid over the bus, stencil, list and block sums on the CPU
    tc, tg, host = [], [], None
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            ages = m.known_age()
            words = m.cast_grid(0)
        t1 = time.perf_counter()
        fr, u, free = R.frontier(unpack(words, w["nx"]), ages, MAX_AGE, MIN_UNKNOWN)
        host = (R.cells(fr), {b: R.blocks(fr, u, b) for b in BLOCKS}, int(free.sum()))
        t2 = time.perf_counter()
        tc.append((t1 - t0) * 1e3)
        tg.append((t2 - t1) * 1e3)
    out["host_ms_copies_stencil_and_sums"] = [round(float(np.median(tc)), 2), round(float(np.median(tg)), 1)]
    out["host_copy_bytes"] = 4 * m.V + words.nbytes
    with torch.cuda.stream(st):
        for b in BLOCKS:
            m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=MIN_UNKNOWN, block=b)
            cells, blocks, counts = m.frontier_cells(), m.frontier_blocks(), m.frontier_counts()
            assert np.array_equal(cells, host[0]), "the device and the host route disagree about the cells (block %d)" % b
            assert blocks.tobytes() == host[1][b].astype(D.capi.FRONTIER_BLOCK_DTYPE).tobytes(), "... about the blocks (block %d)" % b
            assert counts == (len(host[0]), len(host[1][b]), host[2])
            out["block_%d_cells_blocks_free" % b] = list(counts)
    out["cells_of"] = [int(len(host[0])), int(m.V)]

    def arm(b, merge):
        def fn():
            m.set_param(D.capi.P_FRONTIER_MERGE, merge)   # (host state: read when the build is enqueued)
            m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=MIN_UNKNOWN, block=b)
        return fn

    with torch.cuda.stream(st):
        for b in BLOCKS:
            arm(b, 0)()
            assert m.frontier_blocks().tobytes() == host[1][b].tobytes(), "per-cell atomics give other blocks (block %d)" % b
    keys = [("build_block_%d_us_median_min" % b, arm(b, 1)) for b in BLOCKS] + \
           [("build_block_%d_per_cell_atomics_us_median_min" % b, arm(b, 0)) for b in BLOCKS]
    for (k, _), v in zip(keys, timed([fn for _, fn in keys], args.reps)):
        out[k] = v
    m.set_param(D.capi.P_FRONTIER_MERGE, 1)
    with torch.cuda.stream(st):
        assert np.array_equal(m.frontier_cells(), host[0]) and np.array_equal(m.known_age(), ages), "the timed calls changed something"
        # one pass of the loop: frontiers -> block centres -> candidate views -> scores
        t0 = time.perf_counter()
        m.build_frontiers(t=-1.0, max_age=MAX_AGE, min_unknown=MIN_UNKNOWN, block=4)
        c = m.frontier_block_centers(min_count=4)
        views = np.zeros((len(c), 9), np.float32)
        views[:, 0:3], views[:, 3], views[:, 7], views[:, 8] = c, 1.0, 3.0, -1.0
        scores = m.score_views(views, MAX_AGE)
        t1 = time.perf_counter()
    ok = scores["status"] == D.capi.VIEW_OK
    out["loop_views_ok_best_unknown_wall_ms"] = [int(len(c)), int(ok.sum()), int(scores["n_unknown"].max()) if len(c) else 0,
                                                 round((t1 - t0) * 1e3, 2)]
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d" % (args.reps, args.warmup, args.host_reps)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
