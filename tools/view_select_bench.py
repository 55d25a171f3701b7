"""Timing of the joint gain of views (dspmap_select_views_device, dspmap_score_view_sets_device) against dspmap_score_views_device on
the same views -- what the masks and the rounds cost over the stand-alone scores -- and against the route a user has without the
feature: dspmap_debug_view_cells per view (one synchronous copy of a seen set each), dspmap_get_known, and the set cover in numpy
(tests/view_select_ref.greedy_from, the restatement the tests hold the kernels to).  Workloads: config B (66 x 66 x 40 @ 0.15 m, 24
particles / voxel) and 132 x 132 x 60 (9 particles / voxel), each after 20 frames of the synthetic depth stream (scene.py) with
dspmap_known_integrate after every frame, on an unmasked grid (threshold 0.2, inflated by one voxel), max_age 10.

Candidates: the centres of the frontier blocks (dspmap_build_frontiers, block 4) with a random yaw, filled up with random poses inside the
map, all at max_range 3 m, t = -1.  Arms, interleaved call by call:
  a. select_views_device at n = 256 and 4096, k = 4, 16 and 64 (n_fixed 0, min_gain 1)
  b. score_view_sets_device for 256 sets of 8 and of 16 views
  c. score_views_device on the same 256, 2048 and 4096 views
  d. the route without the feature on the first 16 views, k = 4: wall time, median of --host-reps; its figure for 256 views is that
     one scaled, and the output says so.  The tool asserts that both routes give the same picks.
Device times are HIP events on the handle's stream around EVERY one of --reps calls after --warmup untimed ones; median and minimum are
reported.  Also: the bytes of the masks, and the time of one greedy round -- (k = 64 minus k = 16) / 48 -- with the bandwidth the gain
kernel's reads (every candidate's mask once per round) imply.  Prints one JSON line per workload.  bench.py is not involved.

    python tools/view_select_bench.py [--reps 200] [--warmup 3] [--host-reps 3] [--only B|L]
"""
import json
import time

import numpy as np
import torch

import layer_bench as harness
from layer_bench import WORKLOADS

COUNTS = (256, 4096)
PICKS = (4, 16, 64)
SET_SIZES = (8, 16)
N_SETS = 256
MAX_AGE = 10
MAX_RANGE = 3.0
N_HOST, K_HOST = 16, 4


def candidates(w, centres, n, seed):
    """[n, 9]: the frontier block centres first, then random positions inside the map; random yaw, max_range 3 m, t = -1"""
    rng = np.random.default_rng(seed)
    half = np.array([w["nx"], w["ny"], w["nz"]]) * w["res"] * 0.5
    v = np.zeros((n, 9), np.float32)
    v[:, 0:3] = rng.uniform(-0.9, 0.9, (n, 3)) * half
    c = centres[rng.permutation(len(centres))[:n]]
    v[:len(c), 0:3] = c
    yaw = rng.uniform(-np.pi, np.pi, n)
    v[:, 3], v[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    v[:, 7], v[:, 8] = MAX_RANGE, -1.0
    return v, len(c)


def run(D, scene, name, args):
    from tests import reach_ref, view_select_ref
    w = WORKLOADS[name]
    m, st = harness.open_map(D, scene, name, args.frames, after_frame=lambda m: m.integrate_known())
    lw = w["nz"] * w["ny"] * ((w["nx"] + 63) // 64)
    out = {"workload": "%s: %dx%dx%d @ %.2f m, %d particles/voxel" % (name, w["nx"], w["ny"], w["nz"], w["res"], w["ppv"]),
           "state": "%d frames of scene.py, integrated one by one; unmasked grid; max_age %d; max_range %g m" % (args.frames, MAX_AGE, MAX_RANGE),
           "mask_bytes_per_view": lw * 8}
    with torch.cuda.stream(st):
        m.build_cast_grid(0.2, 1)
        m.build_frontiers(max_age=MAX_AGE)
        st.synchronize()
        centres = m.frontier_block_centers()
    views, n_front = candidates(w, centres, max(COUNTS), 7)
    out["frontier_blocks"] = int(len(centres))
    out["candidates_from_frontier_blocks_of_%d" % max(COUNTS)] = int(n_front)
    dviews = torch.from_numpy(views).cuda()
    dsets = {s: dviews[:N_SETS * s].reshape(N_SETS, s, 9) for s in SET_SIZES}
    for n in COUNTS:
        out["mask_bytes_%d_views" % n] = n * lw * 8
    torch.cuda.synchronize()

    def timed(fns, reps):
        return harness.timed(st, fns, reps, args.warmup)

    # d. the route without the feature: a seen set per view over the bus, the ages, the cover in numpy -- and the same picks
    with torch.cuda.stream(st):
        th = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            S = np.stack([reach_ref.unpack(m.view_cells(views[i])[0][None], m.cfg.nx)[0] for i in range(N_HOST)])
            unknown = (lambda a: (a < 0) | (a > MAX_AGE))(m.known_age())
            t1 = time.perf_counter()
            want = view_select_ref.greedy_from(S, unknown, 0, K_HOST, 1)
            t2 = time.perf_counter()
            th.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        got = m.select_views(dviews[:N_HOST], K_HOST, MAX_AGE)
        st.synchronize()
        got = got.cpu().numpy()
        for j, f in enumerate(("view", "gain", "covered")):
            assert np.array_equal(got[:, j], want[f]), "the device and the host route disagree on %s: %s / %s" % (f, got[:, j], want[f])
    copies, cover = (float(np.median([x[i] for x in th])) for i in (0, 1))
    out["host_ms_%d_view_cells_and_ages__numpy_cover_k%d" % (N_HOST, K_HOST)] = [round(copies, 2), round(cover, 2)]
    out["host_ms_scaled_to_256_views_k%d" % K_HOST] = round((copies + cover) * 256 / N_HOST, 1)
    out["picks_of_the_first_%d_views" % N_HOST] = got[:, :3].tolist()

    arms, keys = [], []
    for n in COUNTS:
        for k in PICKS:
            arms.append(lambda n=n, k=k: m.select_views(dviews[:n], k, MAX_AGE))
            keys.append("select_%d_views_k%d_us_median_min" % (n, k))
    for s in SET_SIZES:
        arms.append(lambda s=s: m.score_view_sets(dsets[s], MAX_AGE))
        keys.append("score_%d_sets_of_%d_us_median_min" % (N_SETS, s))
    for n in sorted(set(COUNTS) | set(N_SETS * s for s in SET_SIZES)):
        arms.append(lambda n=n: m.score_views(dviews[:n], MAX_AGE))
        keys.append("score_views_%d_us_median_min" % n)
    res = dict(zip(keys, timed(arms, args.reps)))
    out.update(res)
    for n in COUNTS:
        per_round = (res["select_%d_views_k64_us_median_min" % n][0] - res["select_%d_views_k16_us_median_min" % n][0]) / 48.0
        out["round_us_%d_views" % n] = round(per_round, 2)
        out["gain_kernel_implied_GBps_%d_views" % n] = round(n * lw * 8 / (per_round * 1e-6) / 1e9, 1) if per_round > 0 else None
    sel = m.select_views(dviews[:max(COUNTS)], 16, MAX_AGE, scores=True)
    st.synchronize()
    picks, alone = sel[0].cpu().numpy(), sel[1].cpu().numpy()
    real = picks[picks[:, 0] >= 0]
    out["k16_of_%d_rounds_covered_sum_of_stand_alone" % max(COUNTS)] = [int(len(real)), int(picks[-1, 2]), int(alone[real[:, 0], 1].sum())]
    out["timed_calls"] = "%d after %d untimed, arms interleaved; host route: median of %d on %d views" % (args.reps, args.warmup, args.host_reps, N_HOST)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    m.close()


def main():
    ap = harness.parser(reps=200, warmup=3, frames=20, host_reps=3)
    harness.main(run, ap)


if __name__ == "__main__":
    main()
