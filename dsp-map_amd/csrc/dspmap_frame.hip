// dspmap_frame.hip -- the frame driver of libdspmap_hip.so: DSPMap::update's gating / delta-pose preamble (reference
// include/dsp_dynamic.h:187-218), the launch chain of one frame (enqueue_frame), its capture and replay as a HIP graph, the
// parameter and cloud rings, the host stages, and the reference's stage-by-stage entry points (dspmap_stage_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "dspmap_internal.h"

// --------------------------------------------------------------- the frame
LaunchCtx dspmap_frame_ctx(dspmap* m) {
    LaunchCtx c = dspmap_ctx_of(m);
    if (m->vz_frames <= 0) c.s.vz0 = nullptr;
    return c;
}

void dspmap_freeze_birth_statics(dspmap* m) {
    if (m->nb_frozen) return;
    m->graph_epoch++;  // function statics initialised at first call (:808-811)
    m->fp.min_static_nb = (int)((float)m->fp.nb_num * 0.15f);
    m->fp.model_nb = (int)((float)m->fp.nb_num * 0.8f);
    m->nb_frozen = true;
}

void dspmap_flush_future_clear(dspmap* m) {
    if (!m->fut_clear_pending) return;
    LaunchCtx c = dspmap_ctx_of(m);
    launch_clear_future(c);
    m->fut_clear_pending = false;
}
int dspmap_push_frame_params(dspmap* m) {
    // a pending clear of the future accumulators rides on the frame: its k_predict does it (no extra launch)
    m->hp.clear_fut = m->fut_clear_pending ? 1 : 0;
    m->fut_clear_pending = false;
    m->hp.from_ring = 0;
    // pageable source: the runtime stages the bytes before returning, so m->hp can be reused at once
    HIPCHK(m, hipMemcpyAsync(m->s.fpar, &m->hp, sizeof(FrameParams), hipMemcpyHostToDevice, m->stream));
    return DSPMAP_OK;
}
// A new cloud is about to be binned: bump the frame epoch (FrameScalars::view_epoch refers to it) and return the
// bound for the grids of the birth launches of a synthesised cloud.
int dspmap_begin_cloud(dspmap* m, int n_points, bool static_birth) {
    m->hp.epoch++;
    if (!static_birth) return n_points;
    if (n_points > m->static_hi) m->static_hi = n_points;
    return m->static_hi;
}
static void fill_sensor(dspmap* m) {   // (all a stage that only looks -- dspmap_stage_bin_points -- sets of the pose)
    for (int i = 0; i < 4; i++) m->hp.quat[i] = m->quat[i];
    for (int i = 0; i < 3; i++) m->hp.cur_pos[i] = m->cur_pos[i];
}
// (birth_reach: read by k_tile_class only, which no sharded path launches -- a slab handle carries the value unread)
void dspmap_fill_pose(dspmap* m, const float dp[3], float dt) {
    fill_sensor(m);
    for (int i = 0; i < 3; i++) m->hp.od[i] = -dp[i];  // particles move opposite to the sensor (:300)
    m->hp.dt = dt;
    m->hp.res_filter = m->voxel_filter_res;
    m->hp.birth_reach = m->ptab_max;
}

// A cross-queue wait of an earlier frame gave up (DSPMAP_P_ESTIMATOR_QUEUE; bounded at 200 ms: a contended GPU, a debugger): that frame ran
// WITHOUT its birth stage (k_birth_insert returns when it finds the give-up word: no partial birth cloud is consumed).  Checked by every frame
// entry point BEFORE anything of the handle is touched: the call that finds the note fails once, with the state as the failed frame left
// it, and the handle goes on with the estimator as a forked branch of the graph (xq_failed) -- until the state is cleared or restored or
// the switch is set again.
int dspmap_check_estimator_queue(dspmap* m) {
    if (!m->hint_host || m->hint_host[3] == 0) return DSPMAP_OK;
    const int at = m->hint_host[3] - 1;
    (void)hipStreamSynchronize(m->stream);
    if (m->stream3) (void)hipStreamSynchronize(m->stream3);
    m->hint_host[3] = 0;
    m->xq_failed = true;
    m->graph_epoch++;
    return dspmap_fail(m, DSPMAP_E_DEVICE, "estimator queue: a cross-queue wait gave up at ring position %d; that frame ran without its birth stage, the handle continues with the estimator inside the captured frame (DSPMAP_P_ESTIMATOR_QUEUE)", at);
}

// C0 gate + deltas, update() :187-218.  returns 1 (accepted) / 0 (rejected)
int dspmap_gate_and_delta(dspmap* m, const float pos[3], double stamp, const float q[4], float dp[3], float* dt) {
    if (!m->have_last) {
        m->last_p[0] = pos[0]; m->last_p[1] = pos[1]; m->last_p[2] = pos[2];
        m->last_stamp = stamp;
        m->have_last = true;
    }
    if (fabsf(q[0]) > 1.001f || fabsf(q[1]) > 1.001f || fabsf(q[2]) > 1.001f || fabsf(q[3]) > 1.001f) {
        printf("Invalid quaternion.\n");  // :194
        return 0;
    }
    dp[0] = pos[0] - m->last_p[0]; dp[1] = pos[1] - m->last_p[1]; dp[2] = pos[2] - m->last_p[2];
    *dt = (float)(stamp - m->last_stamp);
    if (fabsf(dp[0]) > 10.f || fabsf(dp[1]) > 10.f || fabsf(dp[2]) > 10.f || *dt < 0.f || *dt > 10.f) {
        printf("!!! delt_t = %f\n", *dt);  // :204-206
        return 0;
    }
    for (int i = 0; i < 3; i++) m->cur_pos[i] = m->last_p[i] = pos[i];
    m->last_stamp = stamp;
    m->dt_last = *dt;
    m->update_time += *dt; m->update_counter += 1;   // mapPrediction :634-635
    dspmap_snapshots_stale(m);   // a new frame: a distance field / cast grid is a snapshot of the one before
    for (int i = 0; i < 4; i++) m->quat[i] = q[i];
    return 1;
}

// does this frame place the arrivals of the tiles with a view first and the others beside the pair kernels / register the movers in k_predict?
static bool frame_splits_placement(const dspmap* m, const LaunchCtx& c) {
    return !m->prof && (!c.sparse || m->place_split_tiles <= 1) && c.k.ntiles >= m->place_split_tiles;   // (1 = always, as documented)
}

// does this frame run as two branches (DSPMAP_P_FRAME_BRANCHES; KernelScratch::tile_cls)?  The same maps that split their placement -- dense and
// large: the branches cost a classification launch and two passes of workgroups over the tiles --, unless forced; never a frame whose
// prediction changes velocities (vz0: constructor-seeded particles draw their noise there, after the classes were sized), a profiled
// frame (one stream), a map that runs the four-waves-per-tile resampler (no class filter there: small maps), or index-order storage
// (MapDims::tiling == 0: a run of 64 voxel indices that points away from the sensor is cut by the field of view almost wherever it
// lies -- 58 % of the 132x132x60 map's runs have a view: there is nothing to leave to a second branch)
static bool frame_runs_two_branches(const dspmap* m, const LaunchCtx& c) {
    if (m->prof || m->frame_branches == 0 || c.s.vz0 || !c.k.tile_cls || !c.d.tiling) return false;   // (cube storage: k_tile_class)
    if (resample_variant(c) & 1) return false;
    return m->frame_branches == 1 || frame_splits_placement(m, c);
}

// does this frame resample the tiles no newborn can reach BESIDE the weight update and the births (DSPMAP_P_RESAMPLE_SPLIT)?  A frame that
// splits its placement (the side stream exists and ends with the placement of exactly such tiles), cube storage (k_tile_class), the
// one-wave-per-tile resampler (class filter), no velocity noise pending, and a birth cloud made on the device from THIS frame's view
// (every point in view a static source, or the device estimator's: a caller-supplied cloud may hold points anywhere)
static bool frame_splits_resampling(const dspmap* m, const LaunchCtx& c, bool split, bool device_cloud) {
    if (!split || m->resample_split == 0 || !device_cloud || c.s.vz0 || !c.k.tile_cls || !c.d.tiling) return false;
    return !(resample_variant(c) & 1);
}

// enqueue one whole device-resident frame (setup .. resample) on the handle's stream, captured or not; every per-frame value is read
// from s.fpar.  One serial chain
//   setup+bin -> predict -> place(view) -> [lists] -> Ck -> weights -> births -> resample
// with up to two side branches on stream2, one behind the other: the device estimator (`est`: from the binning to the birth stage)
// and the placement of the tiles without a view (a frame that splits its placement) -- or, for the maps that ask for it, the
// two-branch frame below.  `all_static`: every point in view is a zero-velocity birth source (the cloud is synthesised).
static void enqueue_frame(dspmap* m, LaunchCtx& c, int pts_grid, int birth_grid, bool all_static, bool est) {
    // (per-stage timing keeps the frame on one stream; so does a sparse map -- most tiles empty: two passes over all the tiles cost
    // more than the overlap gives: 264x264x80 filled by the depth stream 0.445 -> 0.434 ms, 132x132x60 0.232 -> 0.228; saturated
    // maps keep the split: 0.659 against 0.667 ms and 4.61 against 4.80 ms, interleaved runs on one box)
    if (frame_runs_two_branches(m, c)) {
        // TWO BRANCHES (round 6).  The reference's frame is four sweeps over every voxel (:300-322); here most of a large map is only moved
        // and resampled -- bandwidth-bound sweeps -- while pyramid lists, Ck, weights and births (a chain of latency- and VALU-bound
        // kernels) concern the part the sensor sees.  k_tile_class cuts the tiles into that part, grown by the reach of a newborn (Q) and
        // again by the frame's largest displacement (P); then
        //   main:  predict(P) -> place(Q) -> lists -> Ck -> weights -> births -> resample(Q) -+-> rollout
        //   side:  predict(not P) -> [predict(P) done] -> place(not Q) -> resample(not Q) ----+
        // run beside each other.  Same kernels, same per-tile work, same result slot for slot (tests/test_gpu_round6.py).
        c.place_split = false;
        c.branches = true;
        m->rsplit_enq = false;
        if (!m->stream4) {
            // the bulk branch's stream, created at the first frame that needs it, with the LOWEST priority the device offers: its sweeps would
            // otherwise keep every CU's wave slots and LDS filled and the in-view chain's kernels -- the frame's critical path -- would wait
            // for them (list preparation 13 -> 73 us, weights 40 -> 71 us beside them, profiles/r06_b_C_sat_timeline.md)
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            static const bool flat = getenv("DSPMAP_BULK_PRIORITY_FLAT") != nullptr;
            if (flat || hipStreamCreateWithPriority(&m->stream4, hipStreamNonBlocking, lo) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamCreateWithFlags(&m->stream4, hipStreamNonBlocking); }
        }
        launch_setup_and_bin(c, pts_grid, false, m->frame_ring ? m->ring_dev : nullptr, DSPMAP_RING - 1);
        launch_tile_class(c);
        (void)hipEventRecord(m->ev_br[0], m->stream);
        (void)hipStreamWaitEvent(m->stream4, m->ev_br[0], 0);
        LaunchCtx cb = c;
        cb.stream = m->stream4;
        const bool with_est = est && birth_grid > 0;
        const bool early_birth = !with_est && birth_grid > 0;
        launch_predict_only(c, true, early_birth, TILE_P);
        (void)hipEventRecord(m->ev_br[1], m->stream);                 // predict(P) has ended: every arrival of a Q tile is in its inbox
        launch_predict_only(cb, false, false, -TILE_P);
        (void)hipEventRecord(m->ev_br[2], m->stream4);                // predict(not P) has ended: every tile's pending clear is done
        (void)hipStreamWaitEvent(m->stream4, m->ev_br[1], 0);
        launch_claim(cb, 0, 0, 0, 0, -1, -TILE_Q);
        (void)hipEventRecord(m->ev_br[4], m->stream4);                // place(not Q) has ended
        launch_resample(cb, -TILE_Q, false, 2);                       // (the early launch: leaves a frame with an empty view alone, see k_resample)
        (void)hipEventRecord(m->ev_br[3], m->stream4);
        if (with_est) {   // the estimator's branch (the reference's helper thread, :297,311): a third one, from the binning to the birth stage
            (void)hipStreamWaitEvent(m->stream2, m->ev_br[0], 0);
            LaunchCtx c2 = c;
            c2.stream = m->stream2;
            launch_velocity_estimator(c2, true);
            launch_birth_early(c2, birth_grid, false);
            (void)hipEventRecord(m->ev_join, m->stream2);
        }
        launch_claim(c, early_birth ? birth_grid : 0, 0, 0, 0, -1, TILE_Q);
        launch_pyr_prepare(c);
        launch_ck_partial(c, true);
        m->last_weight_variant = launch_weight_update(c);
        if (with_est) {
            (void)hipStreamWaitEvent(m->stream, m->ev_join, 0);
            launch_birth_late(c, birth_grid, false, false);
        } else {
            if (birth_grid <= 0) launch_ck_finalize(c);
            if (early_birth) launch_birth_late(c, birth_grid, all_static);
            else launch_birth(c, birth_grid, true, all_static);
        }
        (void)hipStreamWaitEvent(m->stream, m->ev_br[2], 0);          // (the rollout of the Q tiles adds to accumulators anywhere: after every clear)
        // a frame with an empty view re-uses the birth cloud of the last non-empty one (:1379-1381): its newborns land where THAT frame's
        // field of view was, Q says nothing about them -- this launch then takes every tile, so every tile's placement must have ended
        (void)hipStreamWaitEvent(m->stream, m->ev_br[4], 0);
        launch_resample(c, TILE_Q, false, 4);
        (void)hipStreamWaitEvent(m->stream, m->ev_br[3], 0);
        launch_rollout(c);
        m->last_resample_variant = resample_variant(c);
        m->branch_pending = true;
        return;
    }
    // (DSPMAP_P_TILE_BITMAPS) a sparse unsharded map: the sweeps of this frame find their empty tiles in the bitmaps k_obs_points rebuilds
    c.tile_bits = c.sparse && m->tile_bitmaps && c.k.tile_bits && m->d.v_true == m->d.v_glob && !m->mgpu_bound;
    if (c.tile_bits) {
        const size_t nw = ((size_t)c.k.ntiles + 63) / 64 * 2;
        c.s.vis_bits = c.k.tile_bits; c.s.pred_bits = c.k.tile_bits + nw; c.s.arr_bits = c.k.tile_bits + 2 * nw;
    }
    // Only the arrivals of tiles that can see the field of view are registered in pyramids, so only their placement
    // has to precede the weight update: the others get their slots on the side stream WHILE the pair kernels run
    // (VALU-bound; the list preparation before them is itself a scatter and would only share the memory system).
    const bool split = frame_splits_placement(m, c);
    c.place_split = split;
    // (DSPMAP_P_RESAMPLE_SPLIT) Q = the tiles a newborn of this frame can reach (k_tile_class: the field of view grown by the position
    // table's largest value; every tile with a view is one).  Weights, births and the list re-slotting only touch Q tiles, and the side
    // stream's placement serves exactly the tiles without a view: once it is done the tiles outside Q are final for this frame, and the
    // side stream resamples them while the main chain is still in its weight update and birth stage; the main chain resamples Q behind
    // the births, the rollout follows both.  Same per-tile work, same result slot for slot.
    const bool rsplit = frame_splits_resampling(m, c, split, all_static || est);
    m->rsplit_enq = rsplit;
    // The velocity estimator runs BESIDE prediction and weight update, like the reference's helper thread (:297,311):
    // a second branch of the frame (side stream; a forked branch of the captured graph) takes the binned view through
    // k_ve_components -> k_ve_clusters (+ the birth rank) -> the newborn children, and joins before the birth stage.
    // DSPMAP_P_ESTIMATOR_QUEUE (c.s.xq set; never with a split placement / early registration): no branch at all in this graph -- the caller
    // has queued the estimator's kernels on the other stream itself, k_predict and the split kernel below meet them through DevState::xq
    const bool with_est = est && birth_grid > 0;
    const bool est_branch = with_est && !c.s.xq;
    // births without the estimator: the rank and the children need nothing but the frame's birth cloud -- they ride on the launches of
    // k_predict and k_place and leave the frame's critical path; split, cursors and insert follow the weight update
    const bool early_birth = !with_est && birth_grid > 0;
    // where the side placement leaves the main chain (DSPMAP_P_SIDE_PLACEMENT): 0 behind the list preparation, 1 behind the placement of
    // the tiles with a view, 2 behind the prediction (the side stream carries the estimator first: "behind the prediction" is "behind
    // the placement of the tiles with a view" in a frame with the estimator's branch).  side_leaves(p) before, side_place(p) BEHIND the
    // main chain's next kernel at each of the three points: the branch whose node comes first after the fork stays on the parent's
    // hardware queue, the other one pays the cross-queue hand-over.
    const int side_at = !split ? -1 : (with_est && m->side_fork == 2 ? 1 : m->side_fork);
    auto side_leaves = [&](int p) { if (p == side_at) (void)hipEventRecord(m->ev_fork2, m->stream); };
    auto side_place = [&](int p) {   // the side stream places the arrivals of the tiles outside the field of view (behind the estimator's kernels, if any)
        if (p != side_at) return;
        (void)hipStreamWaitEvent(m->stream2, m->ev_fork2, 0);
        LaunchCtx c2 = c;
        c2.stream = m->stream2;
        if (rsplit) launch_tile_class(c2);
        launch_claim(c2, 0, 0, 0, 0, 0);
        (void)hipEventRecord(m->ev_join, m->stream2);
        if (rsplit) {
            launch_resample(c2, -TILE_Q, false, 2);
            (void)hipEventRecord(m->ev_br[3], m->stream2);
        }
    };
    dspmap_prof_mark(m, 0);
    // the gather rides on k_predict's launch.  (The binning stays on the main chain: as a branch of its own beside prediction and
    // re-binning -- fork=true -- it measured slower: HIP replays multi-branch graphs with a much higher launch cost.)
    launch_setup_and_bin(c, pts_grid, false, m->frame_ring ? m->ring_dev : nullptr, DSPMAP_RING - 1);
    dspmap_prof_mark(m, 1);
    if (est_branch) (void)hipEventRecord(m->ev_fork, m->stream);
    launch_predict_only(c, true, early_birth);   // (queued BEFORE the estimator's branch: see side_place)
    if (est_branch) {
        LaunchCtx c2 = c;
        c2.stream = m->stream2;
        (void)hipStreamWaitEvent(m->stream2, m->ev_fork, 0);
        launch_velocity_estimator(c2, true);
        // the children (the rank ran inside k_ve_clusters): on the side branch when it goes on with the placement of the tiles without
        // a view (large maps); otherwise the branch -- the longer one at the metric's size -- ends here and the waves of the split
        // generate them (launch_birth_late)
        if (split) launch_birth_early(c2, birth_grid, false);
        (void)hipEventRecord(m->ev_join, m->stream2);
    }
    dspmap_prof_mark(m, 2);
    side_leaves(2);
    launch_claim(c, early_birth ? birth_grid : 0, 0, 0, 0, split ? 1 : -1);
    side_place(2);
    side_leaves(1);
    if (split) launch_pyr_prepare(c);
    side_place(1);
    dspmap_prof_mark(m, 3);
    side_leaves(0);
    if (c.pair_self) launch_ck_partial_self(c);   // (never a split placement: k_place's end is this launch's start)
    else launch_ck_partial(c, split);
    side_place(0);
    dspmap_prof_mark(m, 4);
    m->last_weight_variant = launch_weight_update(c, c.pair_self);
    dspmap_prof_mark(m, 5);
    if (with_est ? est_branch : split) (void)hipStreamWaitEvent(m->stream, m->ev_join, 0);   // the side stream's last kernel before the births
    if (!with_est && birth_grid <= 0) launch_ck_finalize(c);   // otherwise k_birth_rank reduces the 1/Ck sums (one launch less)
    dspmap_prof_mark(m, 6);
    if (with_est) launch_birth_late(c, birth_grid, false, !split);
    else if (early_birth) launch_birth_late(c, birth_grid, all_static);
    else launch_birth(c, birth_grid, true, all_static);
    dspmap_prof_mark(m, 7);
    if (!rsplit) dspmap_resample(m, c);
    else {
        m->last_resample_variant = resample_variant(c);
        launch_resample(c, TILE_Q, false, 4);
        (void)hipStreamWaitEvent(m->stream, m->ev_br[3], 0);
        launch_rollout(c);
    }
    dspmap_prof_mark(m, 8);
    if (m->prof) m->prof_pending = true;
}

// The reference keeps ONE clusters_feature_vector_dynamic_last (a function static, :1401,1542).  Here the device estimator
// (dspmap_velest.hip) and the host stage (velocity_estimator.cpp: clouds beyond the device estimator's capacity, or
// DSPMAP_P_VELOCITY_ESTIMATOR = 1) each hold a copy: whenever a frame is about to run on the one that does not hold the
// newer copy, the state is handed over first.
int dspmap_ve_state_to_host(dspmap* m) {
    if (m->ve_last_at != 2) return DSPMAP_OK;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    int n3[4] = {0, 0, 0, 0};
    HIPCHK(m, hipMemcpy(n3, m->ve.n, sizeof(n3), hipMemcpyDeviceToHost));
    const int n = std::max(0, std::min(n3[2], m->ve.cap / 5 + 8));
    std::vector<float> buf((size_t)n * 5 + 1);
    if (n > 0) HIPCHK(m, hipMemcpy(buf.data(), m->ve.last, sizeof(float) * 5 * (size_t)n, hipMemcpyDeviceToHost));
    m->vel.import_last(buf.data(), n);
    m->ve_last_at = 1;
    return DSPMAP_OK;
}
int dspmap_ve_state_to_device(dspmap* m) {
    if (m->ve_last_at != 1) return DSPMAP_OK;
    const int cap = m->ve.cap / 5 + 8;
    std::vector<float> buf((size_t)cap * 5);
    const int n = m->vel.export_last(buf.data(), cap);
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (n > 0) HIPCHK(m, hipMemcpy(m->ve.last, buf.data(), sizeof(float) * 5 * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(m, hipMemcpy(m->ve.n + 2, &n, sizeof(int), hipMemcpyHostToDevice));
    m->ve_last_at = 2;
    return DSPMAP_OK;
}
// the frame's cloud into a pinned staging slot, for the host estimator (m->pts_pin, valid once the stream has passed the copy)
int dspmap_cloud_to_host(dspmap* m, int n, const float* points_dev) {
    int rc = dspmap_pts_slot_acquire(m, n);
    if (rc != DSPMAP_OK) return rc;
    HIPCHK(m, hipMemcpyAsync(m->pts_pin, points_dev, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, m->stream));
    return dspmap_pts_slot_release(m);
}
// the host estimator on the cloud in m->pts_pin (velocityEstimationThread :1377-1544): the tagged birth cloud -> m->h_birth
void dspmap_run_host_estimator(dspmap* m, int n, const float q[4], float dt) {
    std::vector<float> view;
    view.reserve((size_t)n * 3);
    m->vel.rotate_and_filter(m->pts_pin, n, q, view);
    m->vel.run(view, m->cur_pos, dt, m->voxel_filter_res, m->h_birth);
    m->ve_last_at = 1;
}

// The frame's prediction and cloud are queued: one frame less of velocity noise, the cloud's sizes for the birth stage and
// dspmap_get_birth_cloud.
void dspmap_frame_cloud_queued(dspmap* m, int n_points, int n_birth, bool birth_static) {
    if (m->vz_frames > 0) --m->vz_frames;
    m->last_n_points = n_points;
    m->last_n_birth = n_birth;
    m->last_birth_static = birth_static;
}
// A resampling is queued, the frame is complete: the newborn snapshot is spent; `timed`: the closing event of update_ms.
int dspmap_frame_done(dspmap* m, bool timed) {
    if (m->nb_dirty) { m->nb_dirty = false; m->graph_epoch++; }
    if (timed) { HIPCHK(m, hipEventRecord(m->ev1, m->stream)); m->ev_valid = true; }
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}

// One frame with the host stages in the loop (velocity estimator and/or a caller-supplied birth cloud): prediction and
// the weight update are queued first, the host estimator runs while they execute (the reference forks
// velocityEstimationThread before prediction and joins it before the birth stage, :297,311), then the tagged cloud is
// uploaded and birth + resampling follow.  `pts_dev` is the frame's cloud on the device, m->pts_pin its host copy (valid
// once `pts_ready`, if given, has completed).
static int frame_with_host_stages(dspmap* m, int np, const float* pts_dev, const float q[4], const float dp[3], float dt,
                                  hipEvent_t pts_ready) {
    dspmap_freeze_birth_statics(m);
    m->frame_parity ^= 1u;
    LaunchCtx c = dspmap_frame_ctx(m);
    // dsp_static.h has no velocity estimation: every in-FOV point is a zero-velocity birth source
    const bool have_cloud = !m->cfg.static_model && (m->use_vel_est != 0 || m->h_birth_valid);
    dspmap_fill_pose(m, dp, dt);
    m->hp.n_pts = np; m->hp.n_birth = np; m->hp.static_birth = have_cloud ? 0 : 1;
    m->hp.pts = pts_dev; m->hp.birth = m->s.birth;
    const int nb_static_grid = dspmap_begin_cloud(m, np, !have_cloud);
    int rc = dspmap_push_frame_params(m);
    if (rc != DSPMAP_OK) return rc;
    HIPCHK(m, hipEventRecord(m->ev0, m->stream));
    launch_setup_and_bin(c, np, false);
    launch_predict(c, true);
    launch_ck_partial(c);
    m->last_weight_variant = launch_weight_update(c);
    m->last_pair_path = 1;
    int nb = nb_static_grid;
    if (m->use_vel_est != 0 && !m->cfg.static_model) {
        if (pts_ready) HIPCHK(m, hipEventSynchronize(pts_ready));
        rc = dspmap_ve_state_to_host(m);
        if (rc != DSPMAP_OK) return rc;
        dspmap_run_host_estimator(m, np, q, dt);
        m->h_birth_valid = true;
    }
    if (have_cloud) {
        nb = (int)m->h_birth.size();
        rc = dspmap_upload_birth(m, m->h_birth.data(), nb);
        if (rc != DSPMAP_OK) return rc;
        const auto vz0 = c.s.vz0;
        c.s = m->s;  // pointers may have been re-allocated (not vz0: the frame's choice stays)
        c.s.vz0 = vz0;
        m->hp.n_birth = nb; m->hp.birth = m->s.birth;
        rc = dspmap_push_frame_params(m);
        if (rc != DSPMAP_OK) return rc;
    }
    if (nb > 0) launch_birth(c, nb, true, !have_cloud);  // :314-316
    else launch_ck_finalize(c);
    dspmap_resample(m, c);
    dspmap_frame_cloud_queued(m, np, nb, !have_cloud);
    return dspmap_frame_done(m, true);
}

// The frame's parameter block through the pinned ring (m->ring_host must exist) instead of a pageable H2D copy (which makes the host
// wait for the stream to drain: every kernel of the frame is then launched into an empty queue): the frame's first kernel fetches the
// slot over the bus -- no copy node between two graph launches.  Slot k of the ring is reused DSPMAP_RING frames later; an event per
// quarter of the ring makes sure the frames that read it have ended (the host never runs that far ahead in practice).
// dspmap_ring_push() fills the slot from m->hp (the launches then take m->ring_dev); dspmap_ring_pushed() after the frame was queued.
int dspmap_ring_push(dspmap* m) {
    const unsigned q = (m->ring_head / (DSPMAP_RING / 4)) % 4;
    if (m->ring_head % (DSPMAP_RING / 4) == 0 && m->ring_ev_set[q]) HIPCHK(m, hipEventSynchronize(m->ring_ev[q]));
    m->hp.clear_fut = m->fut_clear_pending ? 1 : 0;
    m->fut_clear_pending = false;
    m->hp.from_ring = 1;
    m->hp.ring_pos = m->ring_head;
    m->ring_host[m->ring_head % DSPMAP_RING] = m->hp;
    return DSPMAP_OK;
}
int dspmap_ring_pushed(dspmap* m) {
    if (m->ring_head % (DSPMAP_RING / 4) == DSPMAP_RING / 4 - 1) {
        const unsigned q = (m->ring_head / (DSPMAP_RING / 4)) % 4;
        HIPCHK(m, hipEventRecord(m->ring_ev[q], m->stream));
        m->ring_ev_set[q] = true;
    }
    ++m->ring_head;
    return DSPMAP_OK;
}

// The estimator's own stream (DSPMAP_P_ESTIMATOR_QUEUE), created at the first frame that uses it.  The runtime maps more streams than it has
// hardware queues (GPU_MAX_HW_QUEUES = 4) onto shared ones; if this stream and the handle's main stream land on ONE hardware queue everything
// stays correct (every cross-stream wait is for earlier work) but the estimator runs after the frame instead of beside it (66x66x40: 0.148 ->
// 0.214 ms, seen in bench.py with five streams alive).  So the pairing is TESTED: the main stream is kept busy for 2 ms, a one-microsecond kernel
// goes to the candidate -- if it ends while the main stream is still busy the two do not share a queue; otherwise the candidate is kept aside
// (so that the next one lands elsewhere) and another is tried.  (A high stream priority -- its own pool of hardware queues -- was the first fix:
// with such a stream alive, graph replays WITH a forked branch ran 0.15 ms longer, 132x132x60 saturated + device estimator 0.58 -> 0.73 ms, and
// forking into a prioritised stream during capture crashed the runtime.)
// When NO candidate is apart from the main stream's hardware queue (seen in processes that had created hundreds of streams), the handle does
// not take a shared one (0.214 instead of 0.151 ms per frame at the metric's size): m->xq_shared is set and its frames keep the estimator as
// a forked branch of the captured graph (device_frame).  Test hooks (DSPMAP_XQ_FORCE, read at dspmap_create): "shared" = every candidate counts
// as sharing the queue (the fallback is what runs), "apart" = a handle that finds no candidate apart fails loudly instead of falling back.
static int ensure_estimator_stream(dspmap* m, const LaunchCtx& c) {
    if (m->xq_shared && m->stream3_for == m->stream) return DSPMAP_OK;   // (tested before, for this main stream: nothing apart)
    if (m->stream3 && m->stream3_for == m->stream) return DSPMAP_OK;
    m->xq_shared = false;
    if (m->stream3) { HIPCHK(m, hipStreamSynchronize(m->stream3)); (void)hipStreamDestroy(m->stream3); m->stream3 = nullptr; }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    hipStream_t good = nullptr;
    hipStream_t aside[16]; int n_aside = 0;
    for (int attempt = 0; attempt < (m->xq_force == 2 ? 16 : 6) && !good; ++attempt) {
        hipStream_t cand = nullptr;
        HIPCHK(m, hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
        LaunchCtx cm = c; cm.stream = m->stream;
        LaunchCtx cs = c; cs.stream = cand;
        launch_spin(cm, 2000);
        launch_spin(cs, 1);
        HIPCHK(m, hipStreamSynchronize(cand));
        const bool apart = hipStreamQuery(m->stream) == hipErrorNotReady && m->xq_force != 1;
        (void)hipGetLastError();
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (apart) good = cand; else aside[n_aside++] = cand;
    }
    for (int i = 0; i < n_aside; ++i) (void)hipStreamDestroy(aside[i]);
    m->stream3 = good; m->stream3_for = m->stream;
    if (!good) {   // every candidate shared the main stream's hardware queue: the estimator stays a forked branch of the graph
        m->xq_shared = true;
        if (m->xq_force == 2) return dspmap_fail(m, DSPMAP_E_DEVICE, "estimator queue: no stream apart from the main stream's hardware queue (DSPMAP_XQ_FORCE=apart)");
    }
    return DSPMAP_OK;
}

// The boundary's own call (update(float* host, ...), reference :181): the caller's cloud (m->host_cloud) goes into the slot of the
// mapped cloud ring that belongs to the frame at ring position `pos`, and m->hp.pts points there: k_obs_points fetches it over
// the bus with the parameter block -- the graph launch is the only thing queued for the frame
static int host_cloud_to_ring(dspmap* m, int n_points, unsigned pos) {
    if (!m->cring_host) {
        m->cring_cap = std::max(1, std::min(m->pt_cap, m->ve.cap));   // (this path only carries clouds the device estimator takes: <= ve.cap points; 64 slots x 12 B each)
        HIPCHK(m, hipHostMalloc((void**)&m->cring_host, sizeof(float) * 3 * (size_t)m->cring_cap * DSPMAP_CLOUD_RING, hipHostMallocMapped));
        void* dp2 = nullptr;
        HIPCHK(m, hipHostGetDevicePointer(&dp2, m->cring_host, 0));
        m->cring_dev = (const float*)dp2;
    }
    if (pos >= DSPMAP_CLOUD_RING) {   // the frame that read this slot last must be past its first kernel
        const unsigned need = pos - DSPMAP_CLOUD_RING + 2u;   // (+ 1: the estimator on its own queue reads the slot as well, and is only known to be done with it when the FOLLOWING frame's prediction starts)
        const volatile int* seen = m->hint_host + 2;
        for (long spin = 0; (int)((unsigned)*seen - need) < 0; ++spin) {
            if (spin > 2000) { HIPCHK(m, hipStreamSynchronize(m->stream)); break; }   // (a queue more than 64 frames deep: wait for it)
            std::this_thread::yield();
        }
    }
    float* dst = m->cring_host + (size_t)(pos % DSPMAP_CLOUD_RING) * 3 * (size_t)m->cring_cap;
    const float* src = m->host_cloud;
    const int st = m->host_cloud_stride;
    if (st == 3) memcpy(dst, src, sizeof(float) * 3 * (size_t)n_points);
    else for (int i = 0; i < n_points; i++) {  // xyz are the first three floats of each point (:247,289)
        dst[3 * i] = src[(size_t)i * st]; dst[3 * i + 1] = src[(size_t)i * st + 1]; dst[3 * i + 2] = src[(size_t)i * st + 2];
    }
    m->hp.pts = m->cring_dev + (size_t)(pos % DSPMAP_CLOUD_RING) * 3 * (size_t)m->cring_cap;
    return DSPMAP_OK;
}

// One device-resident frame after the gate (dspmap_update_device; dspmap_update with the device estimator; dspmap_update_depth*).
int dspmap_device_frame(dspmap* m, int n_points, const float* points_dev, int n_birth, const dspmap_vpoint* birth_dev,
                        const float dp[3], float dt, const float q[4]) {
    int rc = dspmap_ensure_point_cap(m, n_points > n_birth ? n_points : n_birth);
    if (rc != DSPMAP_OK) return rc;
    dspmap_freeze_birth_statics(m);
    const bool want_est = !birth_dev && m->use_vel_est != 0 && !m->cfg.static_model;
    const bool est_dev = want_est && m->use_vel_est == 2 && n_points <= m->ve.cap;
    if (want_est && !est_dev && n_points > 0) {
        // device-resident cloud + the HOST velocity estimator (DSPMAP_P_VELOCITY_ESTIMATOR = 1, or a cloud larger than
        // the device estimator orders in one workgroup): the (<= 60 kB) cloud is copied to the host, clustered and
        // matched there WHILE the device predicts and re-weights (the reference's fork/join, :297,311), and the tagged
        // birth cloud is uploaded for the birth stage.
        rc = dspmap_cloud_to_host(m, n_points, points_dev);
        if (rc != DSPMAP_OK) return rc;
        HIPCHK(m, hipEventRecord(m->ev_fork, m->stream));
        dspmap_prof_collect(m);
        rc = dspmap_ve_state_to_host(m);   // (the device estimator may hold the previous frame's clusters)
        if (rc != DSPMAP_OK) return rc;
        return frame_with_host_stages(m, n_points, points_dev, q, dp, dt, m->ev_fork);
    }
    if (est_dev) { if (m->ve_last_at != 2) m->xq_break = true; rc = dspmap_ve_state_to_device(m); if (rc != DSPMAP_OK) return rc; m->ve_last_at = 2; }
    m->frame_parity ^= 1u;
    LaunchCtx c = dspmap_frame_ctx(m);
    const bool has_vz = m->vz_frames > 0;
    // birth cloud: the caller's (0), synthesised from the view (1: every point in view a static source), or the device
    // velocity estimator's (2)
    const int mode = birth_dev ? 0 : (est_dev ? 2 : 1);
    const int nb = mode == 0 ? n_birth : n_points;
    dspmap_fill_pose(m, dp, dt);
    m->hp.n_pts = n_points; m->hp.n_birth = nb; m->hp.static_birth = mode;
    m->hp.pts = points_dev;
    m->hp.birth = mode == 0 ? (BirthSrc*)birth_dev : m->s.birth;
    const int nb_grid = mode != 0 ? dspmap_begin_cloud(m, n_points, true) : (dspmap_begin_cloud(m, n_points, false), nb);
    // a replayed frame reads its parameter block from the pinned ring (dspmap_ring_push)
    m->frame_ring = (m->use_graph || m->direct_ring) && !m->prof && m->ring_host != nullptr;
    // the estimator on a queue of its own (DSPMAP_P_ESTIMATOR_QUEUE): replayed frames with the device estimator whose graph would otherwise fork
    // for it alone -- a split placement / early registration keeps its side branch, and the estimator on it
    bool xq = m->est_queue && !m->xq_failed && m->xq_dev && mode == 2 && m->frame_ring && (m->birth_cap + 15) / 16 + 1 <= DSPMAP_XQ_LIST && !frame_splits_placement(m, c) && !frame_runs_two_branches(m, c);
    if (xq) {   // ... and only on a stream that does not share the main stream's hardware queue (tested once per main stream)
        const int rs = ensure_estimator_stream(m, c);
        if (rs != DSPMAP_OK) return rs;
        if (m->xq_shared) xq = false;
    }
    if (xq) c.s.xq = m->xq_dev;
    if (mode == 2) m->est_path = xq ? 1 : ((m->est_queue && m->xq_shared) ? 2 : 3);
    // (DSPMAP_P_PAIR_PREPARE) a map whose k_weight evaluates every pair needs nothing from k_pyr_prepare while no pyramid list is overfull: its
    // single-chain frames launch the self-mapped pair kernels.  Whether a list IS overfull only the device knows: such a frame sorts and cuts
    // inside the Ck launch (slow, exact) and says so in hint_host[4]; from the first frame that finds the word set the handle prepares its
    // lists again, until its state is cleared or restored.  The choice follows the configuration and that word, never the frame's data.
    if (m->hint_host && m->hint_host[4]) m->pair_sticky = true;
    c.pair_self = m->pair_prepare != 1 && (m->pair_prepare == 2 || !m->pair_sticky) && !m->prof && !m->mgpu_bound &&
                  !frame_splits_placement(m, c) && !frame_runs_two_branches(m, c) && pair_self_legal(c);
    m->last_pair_path = c.pair_self ? 2 : 1;
    if (m->frame_ring && m->host_cloud && n_points > 0) { rc = host_cloud_to_ring(m, n_points, m->ring_head); if (rc != DSPMAP_OK) return rc; }
    rc = m->frame_ring ? dspmap_ring_push(m) : dspmap_push_frame_params(m);
    if (rc != DSPMAP_OK) return rc;
    dspmap_prof_collect(m);
    // update_ms (dspmap_get_counters): an event record between two graph launches costs ~5 us of device time each (measured:
    // 0.162 -> 0.150 ms per frame at the metric's workload without them), so a replayed frame carries the pair only every
    // 32nd time; direct launches (profiling, DSPMAP_P_USE_GRAPH = 0) are timed every frame
    const bool timed = !((m->use_graph || m->direct_ring) && !m->prof) || (m->frame_no++ % 32u) == 0;
    if (timed) HIPCHK(m, hipEventRecord(m->ev0, m->stream));
    auto queue_estimator = [&]() -> int {
        if (!xq) return DSPMAP_OK;
            // this frame's estimator on its own queue, queued BEFORE the frame itself.  It waits for nothing of THIS frame (k_ve_view makes its
            // own picture of the view from the ring slot) -- only for the previous frame's birth stage, which hands over the rand() cursor and
            // the birth buffers: through the word that frame's resampling kernel publishes when that frame was the handle's previous call
            // (nothing else can have touched the estimator's state in between), through an event on the handle's stream otherwise (after
            // another entry point -- a pre-processed cloud, an import, new cursors, a frame of another kind --, or on a stream the caller
            // owns and may have queued the cloud's producer on).  The frame's first birth kernel waits for k_ve_clusters' word.  Every wait
            // is for work queued EARLIER, whatever hardware queues the two streams share: nothing to deadlock on.
            LaunchCtx c2 = c;
            c2.stream = m->stream3;
            if (m->xq_test_break) m->xq_break = true;
            const bool chained = m->own_stream && !m->xq_break && m->xq_chain_api + 1 == m->api_seq;
            m->xq_break = false;
            if (!chained) {
                HIPCHK(m, hipEventRecord(m->ev_fork, m->stream));
                HIPCHK(m, hipStreamWaitEvent(m->stream3, m->ev_fork, 0));
            }
            const int seq = (int)(m->hp.ring_pos + 1u);
            // (test hook: every third frame's estimator is held back by the clock; in the same handles the frame's first birth kernel takes
            // every third frame's cloud for unfinished at its first look whatever the clock says -- DevState::xq[10] -- so that the
            // one-waiting-workgroup / deferred-shares path runs in a known set of frames whichever hardware queues the streams share)
            if (m->xq_test_delay_us > 0 && m->xq_frames % 3 == 1) launch_spin(c2, m->xq_test_delay_us);
            launch_velocity_estimator_xq(c2, true, m->ring_dev + (m->hp.ring_pos % DSPMAP_RING), m->xq_dev, m->s.hint_out + 3, chained ? m->xq_last_seq : 0, seq);
            m->xq_last_seq = seq;
            m->xq_chain_api = m->api_seq;
            ++m->xq_frames;
            return DSPMAP_OK;
    };
    // A two-branch frame is queued as PLAIN launches on the handle's two streams, parameter block through the same pinned ring: replayed as
    // one captured graph its branches did not overlap (the runtime put the bulk branch's prediction behind the in-view chain's birth
    // kernels on one of its internal streams, profiles/r06_*_timeline*), and at this size (0.4 - 5 ms per frame) the ~0.1 ms of host time its
    // fifteen launches take is hidden behind the device
    const bool two = frame_runs_two_branches(m, c);
    // A SMALL map's single-chain frame is queued as plain launches too, by default (DSPMAP_P_USE_GRAPH = 1; 3 keeps the graph): its frame is a
    // serial chain of nine 7 - 29 us kernels, and a replayed linear graph ends with 8.7 us of nothing before the next replay's first kernel --
    // as plain launches (same kernels, parameter block through the same ring, grids sized for the frame's cloud instead of the capacity)
    // k_resample_wg's end is the next k_obs_points' start.  "Single chain": nothing but kernels on the handle's stream (no split placement, no
    // second branch; the estimator on its own queue or absent).  "Small": fewer than DSPMAP_PLAIN_TILES tiles -- larger maps gain 1 % or
    // lose.  NOT the host-pointer update(): its caller pays the launches' host time (~0.1 ms per frame when the queue
    // is deep) in the loop that also copies the cloud, and has been measured host-bound that way; it keeps the one graph launch.
    const bool chain = m->frame_ring && !two && !frame_splits_placement(m, c) && (mode != 2 || xq);
    const bool plain_small = m->graph_mode == 1 && chain && c.k.ntiles < DSPMAP_PLAIN_TILES && !m->host_cloud;
    if (m->use_graph && !m->prof && !two && !plain_small) {
        // the kernel arguments of a frame are constant (per-frame values live in s.fpar): capture once, replay
        const unsigned long long key = ((unsigned long long)m->graph_epoch << 8) | (has_vz ? 1u : 0u) | ((unsigned)mode << 1) | (c.sparse ? 8u : 0u) | (c.ro_inline ? 16u : 0u) | (xq ? 32u : 0u) | (c.pair_self ? 64u : 0u);
        const int gi = c.sweep_rev ? 1 : 0;   // (one executable graph per sweep direction: the direction is a kernel argument)
        if (!m->graph_exec[gi] || m->graph_key[gi] != key) {
            if (m->graph_exec[gi]) {   // (replays of the old executable graph may still be queued: let them finish before it goes)
                HIPCHK(m, hipStreamSynchronize(m->stream));
                (void)hipGraphExecDestroy(m->graph_exec[gi]); m->graph_exec[gi] = nullptr;
            }
            if (m->graph) { (void)hipGraphDestroy(m->graph); m->graph = nullptr; }
            HIPCHK(m, hipStreamBeginCapture(m->stream, hipStreamCaptureModeRelaxed));
            m->graph_rsplit[gi] = false;
            enqueue_frame(m, c, m->pt_cap, m->birth_cap, mode == 1, mode == 2);  // grids sized for the capacity; kernels bound-check against fpar
            HIPCHK(m, hipStreamEndCapture(m->stream, &m->graph));
            m->graph_rsplit[gi] = m->rsplit_enq;
            if (const char* dot = getenv("DSPMAP_GRAPH_DOT")) (void)hipGraphDebugDotPrint(m->graph, dot, 0);   // diagnostics: the frame's nodes and edges
            HIPCHK(m, hipGraphInstantiate(&m->graph_exec[gi], m->graph, nullptr, nullptr, 0));
            (void)hipGraphDestroy(m->graph);   // the executable graph keeps its own copy of the topology
            m->graph = nullptr;
            m->graph_key[gi] = key;
        }
        m->last_resample_variant = resample_variant(c);   // (baked into the graph: c.ro_inline is part of its key)
        rc = queue_estimator();
        if (rc != DSPMAP_OK) return rc;
        HIPCHK(m, hipGraphLaunch(m->graph_exec[gi], m->stream));
        if (m->graph_rsplit[gi]) ++m->rsplit_frames;
    } else {
        if (m->frame_ring) { rc = queue_estimator(); if (rc != DSPMAP_OK) return rc; }
        m->branch_pending = false;
        // plain launches can carry this frame's values as kernel arguments: the block as it stands in the ring slot (dspmap_ring_push)
        if (m->frame_ring) c.hpv = &m->hp;
        enqueue_frame(m, c, n_points, nb_grid, mode == 1, mode == 2);
        if (m->branch_pending) ++m->branch_frames;
        if (m->frame_ring) ++m->plain_frames;
        if (m->rsplit_enq) ++m->rsplit_frames;
    }
    if (m->frame_ring) { rc = dspmap_ring_pushed(m); if (rc != DSPMAP_OK) return rc; }
    dspmap_frame_cloud_queued(m, n_points, nb_grid, mode != 0);   // (mode != 0: the cloud lives on the device, dspmap_get_birth_cloud materialises it)
    return dspmap_frame_done(m, timed);
}

extern "C" int dspmap_update_device(dspmap_t* m, int n_points, const float* points_dev, int n_birth,
                                    const dspmap_vpoint* birth_dev, const float pos[3], double stamp,
                                    const float q[4]) {
    READY(m);
    if (n_points < 0 || (n_points > 0 && !points_dev) || !pos || !q) return dspmap_fail(m, DSPMAP_E_ARG, "bad arguments");
    { const int rq = dspmap_check_estimator_queue(m); if (rq != DSPMAP_OK) return rq; }
    float dp[3], dt;
    if (!dspmap_gate_and_delta(m, pos, stamp, q, dp, &dt)) return DSPMAP_REJECTED;
    return dspmap_device_frame(m, n_points, points_dev, n_birth, birth_dev, dp, dt, q);
}

// The pinned staging buffers rotate: the copy queued from (or into) a slot may still be waiting behind a whole frame when
// the caller comes back with its next cloud, so a slot is refilled only after the event behind its last copy has completed.
int dspmap_pts_slot_acquire(dspmap* m, int n) {
    const unsigned k = m->pts_ring_pos++ % DSPMAP_PTS_RING;
    if (m->pts_ring_busy[k]) { HIPCHK(m, hipEventSynchronize(m->pts_ring_ev[k])); m->pts_ring_busy[k] = false; }
    if (!m->pts_ring_ev[k]) HIPCHK(m, hipEventCreateWithFlags(&m->pts_ring_ev[k], hipEventDisableTiming));
    if (n > m->pts_ring_cap[k] || !m->pts_ring[k]) {
        if (m->pts_ring[k]) (void)hipHostFree(m->pts_ring[k]);
        m->pts_ring[k] = nullptr;
        m->pts_ring_cap[k] = n + n / 2 + 1024;
        HIPCHK(m, hipHostMalloc((void**)&m->pts_ring[k], sizeof(float) * 3 * (size_t)m->pts_ring_cap[k]));
    }
    m->pts_pin = m->pts_ring[k];
    m->pts_pin_cap = m->pts_ring_cap[k];
    return DSPMAP_OK;
}
int dspmap_pts_slot_release(dspmap* m) {
    const unsigned k = (m->pts_ring_pos - 1u) % DSPMAP_PTS_RING;
    HIPCHK(m, hipEventRecord(m->pts_ring_ev[k], m->stream));
    m->pts_ring_busy[k] = true;
    return DSPMAP_OK;
}
int dspmap_stage_points(dspmap* m, int n, int stride, const float* pts) {
    int rc = dspmap_ensure_point_cap(m, n);
    if (rc != DSPMAP_OK) return rc;
    rc = dspmap_pts_slot_acquire(m, n);
    if (rc != DSPMAP_OK) return rc;
    for (int i = 0; i < n; i++) {  // xyz are the first three floats of each point (:247,289)
        m->pts_pin[3 * i] = pts[(size_t)i * stride];
        m->pts_pin[3 * i + 1] = pts[(size_t)i * stride + 1];
        m->pts_pin[3 * i + 2] = pts[(size_t)i * stride + 2];
    }
    if (n > 0) {
        HIPCHK(m, hipMemcpyAsync(m->pts_dev, m->pts_pin, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, m->stream));
        rc = dspmap_pts_slot_release(m);
        if (rc != DSPMAP_OK) return rc;
    }
    return DSPMAP_OK;
}

int dspmap_upload_birth(dspmap* m, const dspmap_vpoint* pts, int n) {
    int rc = dspmap_ensure_point_cap(m, n);
    if (rc != DSPMAP_OK) return rc;
    if (n > m->birth_pin_cap) {
        if (m->birth_ev_set) { HIPCHK(m, hipEventSynchronize(m->birth_ev)); m->birth_ev_set = false; }
        if (m->birth_pin) (void)hipHostFree(m->birth_pin);
        m->birth_pin_cap = n + n / 2 + 1024;
        HIPCHK(m, hipHostMalloc((void**)&m->birth_pin, sizeof(BirthSrc) * (size_t)m->birth_pin_cap));
    }
    static_assert(sizeof(BirthSrc) == sizeof(dspmap_vpoint), "layout");
    if (n > 0) {
        // the previous frame's copy out of this buffer may still be queued behind that frame's kernels
        if (m->birth_ev_set) { HIPCHK(m, hipEventSynchronize(m->birth_ev)); m->birth_ev_set = false; }
        if (!m->birth_ev) HIPCHK(m, hipEventCreateWithFlags(&m->birth_ev, hipEventDisableTiming));
        memcpy(m->birth_pin, pts, sizeof(BirthSrc) * (size_t)n);
        HIPCHK(m, hipMemcpyAsync(m->s.birth, m->birth_pin, sizeof(BirthSrc) * (size_t)n, hipMemcpyHostToDevice, m->stream));
        HIPCHK(m, hipEventRecord(m->birth_ev, m->stream));
        m->birth_ev_set = true;
    }
    return DSPMAP_OK;
}

extern "C" int dspmap_update(dspmap_t* m, int n, int stride, const float* pts, float sx, float sy, float sz,
                             double stamp, float qw, float qx, float qy, float qz) {
    READY(m);
    if (n > 0 && (!pts || stride < 3)) return dspmap_fail(m, DSPMAP_E_ARG, "bad point cloud arguments");
    { const int rq = dspmap_check_estimator_queue(m); if (rq != DSPMAP_OK) return rq; }
    const float pos[3] = {sx, sy, sz};
    const float q[4] = {qw, qx, qy, qz};
    float dp[3], dt;
    if (!dspmap_gate_and_delta(m, pos, stamp, q, dp, &dt)) return DSPMAP_REJECTED;
    const int np = n > 0 ? n : 0;
    const bool dev_frame = m->use_vel_est == 2 && !m->cfg.static_model && !m->h_birth_valid && np <= m->ve.cap;
    if (dev_frame && (m->use_graph || m->direct_ring) && !m->prof && m->ring_host && m->host_direct) {
        // velocity estimator on the device + captured frame: the cloud rides in the pinned cloud ring (device_frame), the frame is one
        // graph launch -- no copy node, no event in front of it (round 4: 5 837 against 6 913 frames/s with the cloud resident in HBM)
        int rc0 = dspmap_ensure_point_cap(m, np);
        if (rc0 != DSPMAP_OK) return rc0;
        m->host_cloud = pts; m->host_cloud_stride = stride;
        rc0 = dspmap_device_frame(m, np, m->pts_dev, 0, nullptr, dp, dt, q);   // (pts_dev: a valid address; replaced by the ring slot when np > 0)
        m->host_cloud = nullptr;
        return rc0;
    }
    int rc = dspmap_stage_points(m, np, stride, pts);
    if (rc != DSPMAP_OK) return rc;
    m->xq_break = true;   // (the cloud reaches pts_dev through a copy on the handle's stream)
    if (dev_frame)
        return dspmap_device_frame(m, np, m->pts_dev, 0, nullptr, dp, dt, q);   // velocity estimator on the device: no host stage in the frame
    return frame_with_host_stages(m, np, m->pts_dev, q, dp, dt, nullptr);
}

extern "C" int dspmap_set_birth_cloud(dspmap_t* m, const dspmap_vpoint* pts, int n) {
    if (!m || n < 0 || (n > 0 && !pts)) return DSPMAP_E_ARG;
    m->h_birth.assign(pts, pts + n);
    m->h_birth_valid = true;
    return DSPMAP_OK;
}
extern "C" int dspmap_get_birth_cloud(dspmap_t* m, dspmap_vpoint* out, int cap, int* n_out) {
    READY(m);
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (m->last_birth_static) {
        // the synthesised cloud is rebuilt from the frame's view (or is the kept cloud of the last non-empty view)
        BirthSrc* dtmp = nullptr;
        int* dn = nullptr;
        const int capb = m->pt_cap > 0 ? m->pt_cap : 1;
        HIPCHK(m, hipMalloc((void**)&dtmp, sizeof(BirthSrc) * (size_t)capb));
        HIPCHK(m, hipMalloc((void**)&dn, sizeof(int)));
        LaunchCtx c = dspmap_ctx_of(m);
        launch_birth_materialize(c, dtmp, capb, dn);
        int nsrc = 0;
        HIPCHK(m, hipMemcpyAsync(&nsrc, dn, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (nsrc > capb) nsrc = capb;
        std::vector<BirthSrc> tmp((size_t)nsrc);
        if (nsrc) HIPCHK(m, hipMemcpy(tmp.data(), dtmp, sizeof(BirthSrc) * tmp.size(), hipMemcpyDeviceToHost));
        (void)hipFree(dtmp); (void)hipFree(dn);
        int k = 0;
        for (auto& b : tmp)
            if (b.intensity > -1.5f) { if (out && k < cap) memcpy(&out[k], &b, sizeof(b)); ++k; }
        if (n_out) *n_out = k;
    } else {
        const int n = (int)m->h_birth.size();
        for (int i = 0; i < n && i < cap && out; i++) out[i] = m->h_birth[i];
        if (n_out) *n_out = n;
    }
    return DSPMAP_OK;
}

// ------------------------------------------------------------------ stages
extern "C" int dspmap_stage_bin_points(dspmap_t* m, int n, int stride, const float* pts, float qw, float qx, float qy, float qz) {
    READY(m);
    if (n < 0 || (n > 0 && (!pts || stride < 3))) return DSPMAP_E_ARG;
    m->quat[0] = qw; m->quat[1] = qx; m->quat[2] = qy; m->quat[3] = qz;
    int rc = dspmap_stage_points(m, n, stride, pts);
    if (rc != DSPMAP_OK) return rc;
    LaunchCtx c = dspmap_ctx_of(m);
    fill_sensor(m);
    m->hp.n_pts = n; m->hp.n_birth = n; m->hp.static_birth = m->h_birth_valid ? 0 : 1;
    m->hp.pts = m->pts_dev; m->hp.birth = m->s.birth;
    const int nb_grid = dspmap_begin_cloud(m, n, !m->h_birth_valid);
    rc = dspmap_push_frame_params(m);
    if (rc != DSPMAP_OK) return rc;
    launch_frame_setup(c, true);
    launch_obs_bin(c, n);
    m->last_n_points = n;
    if (!m->h_birth_valid) { m->last_n_birth = nb_grid; m->last_birth_static = true; }
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_set_current_position(dspmap_t* m, float x, float y, float z) {
    if (!m) return DSPMAP_E_ARG;
    m->cur_pos[0] = x; m->cur_pos[1] = y; m->cur_pos[2] = z;
    dspmap_layers_stale(m->ly, LAYERS_POSITION_CHANGED);   // (frontiers are found in the known-space window of the position they were built at)
    return DSPMAP_OK;
}
extern "C" int dspmap_stage_predict(dspmap_t* m, float dx, float dy, float dz, float dt) {
    READY(m);
    dspmap_snapshots_stale(m);
    m->frame_parity ^= 1u;
    LaunchCtx c = dspmap_frame_ctx(m);
    fill_sensor(m);   // (not dspmap_fill_pose: the stage leaves res_filter and birth_reach as they are)
    m->hp.od[0] = dx; m->hp.od[1] = dy; m->hp.od[2] = dz; m->hp.dt = dt;
    m->update_time += dt; m->update_counter += 1;   // :634-635
    if (!m->hp.birth) m->hp.birth = m->s.birth;
    { int rc = dspmap_push_frame_params(m); if (rc != DSPMAP_OK) return rc; }
    launch_frame_setup(c, false);
    launch_predict(c);
    launch_pyr_prepare(c);   // a full pyramid list turns its latest particles (in sweep order) away: part of the prediction (:1256-1259)
    launch_place_fix(c);     // ... and the arrivals behind a turned-away particle take the slot it hands back
    if (m->vz_frames > 0) --m->vz_frames;
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_stage_update(dspmap_t* m) {
    READY(m);
    dspmap_snapshots_stale(m);
    LaunchCtx c = dspmap_ctx_of(m);
    launch_ck_partial(c);
    m->last_weight_variant = launch_weight_update(c);
    m->last_pair_path = 1;
    launch_ck_finalize(c);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_stage_birth(dspmap_t* m) {
    READY(m);
    dspmap_snapshots_stale(m);
    dspmap_freeze_birth_statics(m);
    int nb = m->last_n_birth;
    if (m->h_birth_valid) {
        nb = (int)m->h_birth.size();
        int rc = dspmap_upload_birth(m, m->h_birth.data(), nb);
        if (rc != DSPMAP_OK) return rc;
        m->last_birth_static = false;
        m->last_n_birth = nb;
    }
    LaunchCtx c = dspmap_frame_ctx(m);
    for (int i = 0; i < 3; i++) m->hp.cur_pos[i] = m->cur_pos[i];
    m->hp.n_birth = nb; m->hp.birth = m->s.birth;
    m->hp.static_birth = m->last_birth_static ? 1 : 0;   // a cloud supplied after the binning replaces the synthesised one
    { int rc = dspmap_push_frame_params(m); if (rc != DSPMAP_OK) return rc; }
    launch_birth(c, nb, false, false);
    HIPCHK(m, hipGetLastError());
    return dspmap_mark_nb_dirty(m);   // until a resampling turns the newborn flags into 1 (:968)
}
extern "C" int dspmap_stage_resample(dspmap_t* m) {
    READY(m);
    dspmap_snapshots_stale(m);
    dspmap_flush_future_clear(m);   // a pending clear must not wipe what this stage accumulates
    LaunchCtx c = dspmap_frame_ctx(m);
    dspmap_resample(m, c);
    return dspmap_frame_done(m, false);   // (the stages carry no update_ms)
}
