// dspmap_kernels.h -- launchers of the gfx950 kernels (host-callable).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dspmap_types.h"

// scratch owned by the runtime
struct KernelScratch {
    float4* mv_rec;     // [ntiles][64*slots][2] per-source-tile staging of k_predict (movers up, in-FOV stayers down)
    unsigned long long* vz_q;       // [v_loc*mw] (with vz0) slots that draw velocity noise in their first prediction
    unsigned long long* omask;      // [v_loc*mw] occupancy (mask | nbmask) before the frame's prediction (k_predict -> k_place)
    float4* in_rec;     // [ntiles][64*slots][2] per-destination-tile inbox of movers (k_predict tail -> k_place)
    int* in_cnt;        // [ntiles] inbox fill; zeroed again by k_place
    unsigned* tile_bits;  // [3][(ntiles + 63) / 64 * 2] the tile bitmaps (DevState::vis_bits / pred_bits / arr_bits point into it while they are in use)
    u64* expmask;       // [v_loc*mw] particles that left the slab (multi-GPU), or nullptr
    int* part_predict;  // [ntiles*4]
    int* tile_fov;      // [ntiles] 1 = a particle inside this tile may lie in the field of view (k_predict, conservative box test):
                        // the placement of the other tiles registers nothing in a pyramid and may run beside the pair kernels
    int* view_list;     // [ntiles] the tiles with a view on the field of view this frame, in no particular order (FrameScalars::n_view_tiles of them):
                        // written by extra workgroups of k_predict when the frame splits its placement, walked by the placement that precedes
                        // the pair kernels INSTEAD of all the tiles
    int* tile_cls;      // [ntiles] the TWO-BRANCH frame's tile classes, written by k_tile_class right after the binning (LaunchCtx::branches):
                        // bit 0 (Q) = a newborn of this frame can land in the tile (its rows, grown by the position table's reach, touch the field
                        // of view) -- and every tile in which a particle can be registered in a pyramid; bit 1 (P) = a particle of the tile can
                        // reach a Q tile this frame (Q's rows dilated by the frame's largest displacement).  The in-view chain predicts P,
                        // places and resamples Q; the bulk branch predicts / places / resamples the complements beside it
    int* part_resample; // [ntiles rounded up to 4] live particles per tile after resampling
    int* vb_cnt;        // [v_loc] children per destination voxel this frame (birth ordering)
    int* vb_idx;        // [v_loc*128] their birth indices
    int* ck_items;      // [np * (ceil(capp/32)+1)] work items of k_ck_partial (pyramid<<12 | chunk)
    int* wu_items;      // [np * (ceil(capp/256)+1)] work items of k_weight
    int* n_items;       // [4] Ck items, weight items, particles per Ck item (dspmap_debug_pair_items); [3] workgroups of an overfull self-mapped Ck launch that are done
    int* nb_tab;        // [NB_TAB_STRIDE][np] neighbourhood of every pyramid: bins (h-major, -1 padded) + exclusive offsets of
                        // their observation counts, written by k_pyr_items once per frame
    int* part_birth;    // [ceil(birth_cap*32/256)*2] per-block {born, dropped} of k_birth_insert
    float4* child;      // [birth_cap*32] child position + destination voxel of this frame's births
    u64* nbsnap;        // [v_loc*mw] newborn bits as they were BEFORE this frame's birth stage, or nullptr when they are known
                        // to be all zero (every frame after a resampling).  Non-null after a constructor pre-fill / an import of
                        // flag-15 records / a second birth stage without resampling: addAParticle (:1184-1185) skips those slots
    float4* ro_rec;     // [ntiles][64*slots][2] the tile's MOVING old particles {px, py, vx, vy}, {w, local voxel} (k_resample -> k_rollout)
    int* ro_cnt;        // [2 * ntiles] per tile: records in ro_rec; then the float bits of their summed weight
    int* ro_sub;        // [4 * ntiles] (cube storage) lengths of the four runs -- one per layer of the cube -- k_resample writes a tile's records
                        // in; [4 t] = -1: ONE mixed run of ro_cnt[t] records (k_resample_wg)
    int* ro_stat;       // [2 * ceil(ntiles / 8)] per group of k_rollout: contributions through its LDS windows / straight to the accumulators
    int* work_list;     // [v_loc] scratch: per-voxel prefix of the constructor-seeded particles' noise ranks (k_vz_count)
    int ntiles;         // tiles of 64 voxels; k_predict / k_place run one workgroup per tile
    int nblk_sweep;
};

struct LaunchCtx {
    MapDims d;
    FilterParams fp;
    DevState s;
    KernelScratch k;
    hipStream_t stream;
    int pt_cap, birth_cap;
    VelEst ve;
    int n_cu = 256;      // compute units of the device (sizes launches that are meant to occupy only a share of it)
    bool ro_inline = true; // small maps (k_resample_wg): the tiles roll their moving particles out themselves, no k_rollout launch
    int resample_wg_tiles = 8192;   // one-word maps with fewer tiles (and sparse ones of any size) run k_resample_wg (dspmap::resample_wg_tiles, DSPMAP_P_RESAMPLE_WG_TILES)
    bool sweep_rev = false;   // this frame's k_predict / k_resample walk the tiles from the last one down and k_place from the first one up
                              // (the next frame the other way round): every tile sweep starts where its predecessor ended (Infinity Cache)
    bool resample_rev = false;   // k_resample walks the tiles from the last one down (after a k_place that ended there)
    bool place_split = false; // this frame places the arrivals of the tiles with a view first (launch_claim sel = 1) and the others beside the pair
                              // kernels (sel = 0): k_predict leaves the list of the tiles with a view (KernelScratch::view_list)
    bool tile_bits = false;   // this frame's sweeps go by the tile bitmaps (sparse whole frames of an unsharded map; DSPMAP_P_TILE_BITMAPS)
    int side_wg = 3;          // workgroups per CU of the side-stream placement (sel = 0; DSPMAP_P_SIDE_PLACEMENT)
    bool pair_self = false;  // this frame's pair kernels map their items themselves and read the lists as registered: no k_pyr_prepare (DSPMAP_P_PAIR_PREPARE)
    bool branches = false;   // this frame runs as two branches (DSPMAP_P_FRAME_BRANCHES; see KernelScratch::tile_cls)
    bool sparse = false; // most tiles hold nothing (dspmap::sparse_mode): k_predict's variant that leaves such tiles first
    const FrameParams* hpv = nullptr;   // (host memory) a frame queued as PLAIN launches through the parameter ring: the block that was just pushed into its ring
                                        // slot -- the frame's first kernel takes it as a kernel argument instead of reading it back over the bus.
                                        // nullptr: a captured frame (frozen arguments), or no ring
};

// frame setup: rotate boundary planes (:226-232), reset per-frame counters/bins (:235-238)
void launch_frame_setup(const LaunchCtx& c, bool reset_obs);
// observation binning (:244-290)
void launch_obs_bin(const LaunchCtx& c, int n_pts_grid);
void launch_setup_and_bin(const LaunchCtx& c, int n_pts_grid, bool gather = true, const FrameParams* ring = nullptr, int ring_mask = 0);   // ring: the frame's parameter block is read from this pinned ring   // gather = false: launch_predict*(c, true) does it
// mapPrediction (:627-701) incl. re-binning of movers (moveParticle :1206-1274)
void launch_predict(const LaunchCtx& c, bool with_gather = false);
void launch_spin(const LaunchCtx& c, int us);   // experiment aid: a one-wave kernel that waits `us` microseconds
void launch_predict_only(const LaunchCtx& c, bool with_gather = false, bool with_rank = false, int cls = 0);   // with_rank: k_birth_rank rides along
   // cls (two-branch frame): 0 every tile; +m only the tiles whose class has a bit of m, -m only those that have none (KernelScratch::tile_cls)
void launch_tile_class(const LaunchCtx& c);   // after the binning (needs the rotated planes and the frame's parameter block)
#define TILE_Q 1
#define TILE_P 2
void launch_scan_blocks(const LaunchCtx& c, int nblk);   // exclusive scan of s.blk_cnt[0..nblk), total -> fs->occupied_count
void launch_claim(const LaunchCtx& c, int n_birth_grid = 0, int part = 0, int tile_lo = 0, int tile_hi = 0, int sel = -1, int cls = 0);   // sel: -1 every tile of the part, 1 / 0 only the tiles with / without a view on the sensor's field of view (tile_fov)   // part: 0 all tiles, 1 [lo, hi), 2 the rest;   // > 0: k_birth_children rides along (after a launch with_rank)
void launch_reduce_counters(const LaunchCtx& c);
void launch_calib(const LaunchCtx& c, int mode, size_t n);
void launch_sweep_probe(const LaunchCtx& c, int what, int rows, int rows_per_batch);
// every float a in [0, amax]: does reciprocal + two FMAs give the IEEE quotient a / res?  *bad counts the exceptions
void launch_verify_div(hipStream_t stream, float res, float rcp_res, float amax, int* bad);
// multi-GPU: compact particles that left the slab / insert particles received from a neighbour
void launch_export_slab(const LaunchCtx& c, int dir, float* rec_out, int cap, int* count_dev, float* rec_out_down = nullptr);   // dir 0: both (up -> rec_out / count[0], down -> rec_out_down / count[1])
void launch_import_movers(const LaunchCtx& c, int n, const float* rec);  // folds the per-block partial counters into FrameScalars
// velocityEstimationThread (:1377-1544) on the device: view -> birth cloud in DevState::birth, FrameScalars::est_n
void launch_velocity_estimator(const LaunchCtx& c, bool with_rank);   // with_rank: + the birth stage's rank in the same workgroup
// ... on a queue of its own (c.stream = that queue; DevState::xq): k_ve_view (waits for "the previous frame's birth stage has ended" unless want
// == 0, then rotates and bins the view from the frame's ring slot), the two kernels on that picture, and the word the frame's first birth kernel
// waits for (= xq_seq)
void launch_velocity_estimator_xq(const LaunchCtx& c, bool with_rank, const FrameParams* slot, int* xq, int* gave_up, int want, int xq_seq);
int velocity_estimator_capacity();   // points per frame the device estimator handles
int velocity_estimator_slices();
// mapUpdate (:704-793)
void launch_place_fix(const LaunchCtx& c);     // re-slots the arrivals of voxels in which a full pyramid list turned a particle away (after launch_pyr_prepare)
// sharded maps: one pass (8 bits, most significant first) of the distributed selection of every pyramid's CAPP-th smallest sweep key;
// the caller sums `hist` ([np][256]) over the ranks between the two launches
void launch_pyr_hist(const LaunchCtx& c, int pass, const int2* sel, int* hist);
void launch_pyr_pick(const LaunchCtx& c, int pass, const int* hist, int2* sel, int* kstar);
int pyr_select_passes();
void launch_pyr_kept(const LaunchCtx& c, const int* kstar, int* kept);   // after the last pass: this rank's kept entries per pyramid
void launch_pyr_prepare(const LaunchCtx& c);   // range sort + full-list selection of the pyramid lists, work items (idempotent)
void launch_ck_partial(const LaunchCtx& c, bool prepared = false, bool with_fix = true);   // with_fix: the first workgroups run k_place_fix's pass     // launch_pyr_prepare (unless already queued) + the Ck pass
void launch_ck_finalize(const LaunchCtx& c);
bool pair_self_legal(const LaunchCtx& c);        // this configuration can run the self-mapped pair kernels: every pair evaluated, unsharded, np and capp within their LDS tables
void launch_ck_partial_self(const LaunchCtx& c);   // the Ck pass on the lists as registered: no launch_pyr_prepare; overfull lists are sorted, cut and re-slotted by its extra workgroups
int launch_weight_update(const LaunchCtx& c, bool self = false);   // self: after launch_ck_partial_self (only where pair_self_legal);   // returns which k_weight it launched: 1 = <false> (every pair evaluated, far ones masked), 2 = <true> (far pairs branched over)
// mapAddNewBornParticlesByObservation (:796-921)
void launch_birth(const LaunchCtx& c, int n_birth, bool in_frame, bool all_static);  // in_frame: between k_weight and k_resample of a whole frame
void launch_birth_split(const LaunchCtx& c, int n_birth);
void launch_birth_split_cksum(const LaunchCtx& c, int n_birth);             // split + the 1/Ck reduction in one launch
void launch_birth_early(const LaunchCtx& c, int n_birth, bool with_rank = true);                      // split-phase frame: rank + children right after the prediction
void launch_birth_finish(const LaunchCtx& c, int n_birth, bool all_static);    // ... cursors + insert at its end
void launch_birth_late(const LaunchCtx& c, int n_birth, bool all_static, bool with_children = false);   // with_children: no k_birth_children launch preceded (the split's waves generate them);   // whole frame after launch_predict_only(with_rank) + launch_claim(n): split, 1/Ck sum, cursors, insert
void launch_birth_plan_insert(const LaunchCtx& c, int n_birth, bool in_frame, bool all_static);
void launch_birth_materialize(const LaunchCtx& c, BirthSrc* out, int cap, int* n_out);   // the frame's synthesised birth cloud, for host readback
// mapOccupancyCalculationAndResample (:924-1057)
void launch_resample(const LaunchCtx& c, int cls = 0, bool with_rollout = true, int part = 0);   // + the future rollout of the moving particles (k_rollout)
int rollout_groups(const MapDims& d, int ntiles);   // workgroup groups of k_rollout (KernelScratch::ro_stat holds 2 ints per workgroup: x 4 with cube storage and windows)
int rollout_plan_halos(const MapDims& d, int* halo_out);   // k_rollout's window plan for this map: halo rows per horizon -> halo_out[T]; returns the LDS cells of all windows
void launch_rollout(const LaunchCtx& c);    // the rollout alone (a two-branch frame: once, behind both branches' resampling)
int resample_variant(const LaunchCtx& c);   // bit 0: k_resample_wg; bits 1-2: rollout 0 inline, 1 k_rollout light, 2 k_rollout windows, 3 none
void kernels_init_device();                 // function attributes of the current device (dynamic LDS of k_rollout)
// readout (:385-438)
void launch_occupied_compact(const LaunchCtx& c, float thr);
void launch_clear_future(const LaunchCtx& c);
void launch_future_combine(const LaunchCtx& c);  // fold the static-particle future mass into the [V][T] grid
void launch_results_true(const LaunchCtx& c, float4* out);   // res4 (storage order) -> the reference's voxel order
// point / trajectory queries (dspmap_query.hip; semantics in include/dspmap.h, dspmap_query_occupancy)
// the frame of a batch's samples.  It opens every argument block that takes samples (asserted next to each), so a kernel reads its other
// arguments where it did when these were four loose fields
struct SampleOrigin {
    float ox, oy, oz;    // subtracted from every sample when `world` is set: the sensor position of the last update (current_position :131)
    int world;
};
static_assert(sizeof(SampleOrigin) == 16, "SampleOrigin is the 16 bytes of the four fields it replaces");
struct QueryArgs {
    SampleOrigin org;
    float r2;           // fl(r * r)
    int K;               // lattice steps either side of a sample's own lattice cell the candidate box spans; 0 = the own voxel only (r == 0)
    float outside;       // what a lattice point outside the map, a point outside it or a NaN input contributes
    int fut_zero;        // 1: a clear of the future accumulators is pending -- t >= 0 reads 0
    float cx, cy, cz;    // -half + res / 2 per axis: the voxel centre of index i is fl(fl(i * res) + c) (dspmap_voxel_center)
};
struct dspmap_risk;
// out[i] = the value of sample q[i]; out_flag (optional) = 1 where the point is outside the map or an input is NaN
void launch_query(const LaunchCtx& c, const QueryArgs& a, int n, const float4* q, float* out, unsigned char* out_flag);
// per trajectory of n_samples consecutive values: sequential fp32 sum, max, first value > threshold, flagged samples
void launch_risk_reduce(const LaunchCtx& c, int n_traj, int n_samples, const float* v, const unsigned char* flag, float threshold,
                        struct dspmap_risk* out);
// truncated Euclidean distance fields of the current and the predicted occupancy (dspmap_distance.hip; semantics in include/dspmap.h,
// dspmap_build_distance_field).  Three separable passes over all L = T + 1 layers at once; the grids are in the reference's voxel order
struct DistArgs {
    float thr;           // a voxel is occupied iff its mass > thr (getOccupancyMap's comparison, :394)
    int R;               // truncation radius in voxels, 1 .. 64
    int outside_occ;     // DSPMAP_DIST_OUTSIDE_OCCUPIED: the lattice just outside the map counts as occupied
    int fut_zero;        // 1: a clear of the future accumulators is pending -- the layers >= 1 are empty
    int L;               // layers: T + 1
    unsigned char* g8;   // [L][V] pass 1: distance along x to the row's nearest occupied voxel, clamped to R + 1
    unsigned short* h16; // [L][V] pass 2: squared distance within the z plane, clamped to R^2
    float* field;        // [L][V] pass 3: the field
};
void launch_distance_field(const LaunchCtx& c, const DistArgs& a);
struct DistQueryArgs {
    SampleOrigin org;
    float outside;       // what a point outside the map or a NaN sample reads
    const float* field;  // [L][V]
};
// dist[i] = the field at sample q[i]'s own voxel in the layer its t selects, grad[3 i ..] (optional) = its central / one-sided differences
void launch_distance_query(const LaunchCtx& c, const DistQueryArgs& a, int n, const float4* q, float* dist, float* grad);
// nearest-obstacle fields: the distance transform with its argmin carried through the passes (dspmap_nearest.hip; semantics in
// include/dspmap.h, dspmap_build_nearest_field).  VL virtual layers per launch: the L layers and, signed, their L complements behind them
struct NearArgs {
    float thr;           // a voxel is occupied iff its mass > thr (as DistArgs); not read when `grid` is set
    int R;               // truncation radius in voxels, 1 .. 64
    int sgn;             // DSPMAP_NEAREST_SIGNED: occupied cells target the free voxels, their distance is negated
    int fut_zero;        // 1: a clear of the future accumulators is pending -- the layers >= 1 are empty
    int L;               // layers: T + 1
    const u64* grid;     // DSPMAP_NEAREST_FROM_CAST_GRID: [L][nz][ny][W] the cast grid, else NULL (the masses decide)
    signed char* x8;     // [VL][V] pass 1: ux - x of the row's nearest target, NEAR_NONE8 beyond R
    unsigned* key32;     // [VL][V] pass 2: (D2 within the z plane << 16) | (uy - y) << 8 | (ux - x), D2 = 0x7fff for none
    int* near;           // [L][V] pass 3: global index of the nearest target, -1 for none
    float* dist;         // [L][V] pass 3: the (signed) distance
};
void launch_nearest_field(const LaunchCtx& c, const NearArgs& a);
struct NearQueryArgs {
    SampleOrigin org;
    float outside;       // what a point outside the map or a NaN sample reads
    float cx, cy, cz;    // as QueryArgs: dspmap_voxel_center
    const int* near;     // [L][V]
    const float* dist;   // [L][V]
};
struct dspmap_nearest;
void launch_nearest_query(const LaunchCtx& c, const NearQueryArgs& a, int n, const float4* q, struct dspmap_nearest* out);
// segment casts through a bit grid of the current and the predicted occupancy (dspmap_cast.hip; semantics in include/dspmap.h,
// dspmap_build_cast_grid).  The grid is in the reference's voxel order: [L][nz][ny][W] words, W = ceil(nx / 64)
struct CastGridArgs {
    float thr;           // a voxel is occupied iff its mass > thr (as DistArgs)
    int r;               // Chebyshev inflation radius in voxels, 0 .. DSPMAP_CAST_MAX_INFLATE
    int fut_zero;        // 1: a clear of the future accumulators is pending -- the layers >= 1 are empty
    int L;               // layers: T + 1
    u64* bits;           // [L][nz][ny][W] the grid
    u64* tmp;            // the same size: the grid after the x and y passes of the inflation
};
void launch_cast_grid(const LaunchCtx& c, const CastGridArgs& a);
struct CastArgs {
    SampleOrigin org;
    const u64* bits;     // [L][nz][ny][W]
};
struct dspmap_segment;
struct dspmap_cast_hit;
void launch_cast(const LaunchCtx& c, const CastArgs& a, int n, const struct dspmap_segment* seg, struct dspmap_cast_hit* out);
// axis-aligned free boxes grown in the cast grid, one wave per seed (dspmap_corridor.hip; semantics in include/dspmap.h, dspmap_grow_boxes)
struct BoxArgs {
    SampleOrigin org;
    int with_current;    // DSPMAP_BOX_WITH_CURRENT: layer 0 is tested in addition
    int grow[3];         // max_grow per axis, 0 .. DSPMAP_BOX_MAX_GROW
    const u64* bits;     // [L][nz][ny][W]
};
struct dspmap_box;
void launch_grow_boxes(const LaunchCtx& c, const BoxArgs& a, int n, const struct dspmap_segment* seed, struct dspmap_box* out);
// arrival-time fields: a space-time wavefront through the cast grid, one workgroup per field (dspmap_reach.hip; semantics in include/dspmap.h,
// dspmap_build_reach_fields)
struct ReachArgs {
    SampleOrigin org;
    int with_current;    // DSPMAP_REACH_WITH_CURRENT: layer 0 is tested in addition
    int timed;           // t_start >= 0 and T > 0: step n tests layer 1 + k(t_n); otherwise every step tests layer 0
    float t_start, step_seconds;
    int max_steps;
    int n_fix;           // the first step from which the tested layer no longer changes (host: the schedule is walked once)
    int n_fields, n_src;
    const u64* bits;     // [L][nz][ny][W]
    unsigned short* field;   // [n_fields][V], preset to DSPMAP_REACH_UNREACHED
    u64* sets;           // [n_fields][2][nz * ny * W] device scratch of the two wave sets, or nullptr: they live in LDS
};
struct FieldPathArgs {           // dspmap_reach_paths and dspmap_cost_paths: the descent through a field's values
    SampleOrigin org;
    int n_fields, max_len;
    const unsigned short* field;
    const unsigned char* weight; // [V] the cost build's weights: the step out of cell g is weight[g]; not read by the reach paths (step 1)
};
struct ReachTimelinePathArgs {   // dspmap_reach_timeline_paths: backwards through the sets a timeline build kept
    SampleOrigin org;
    int n_fields, max_len;
    int max_steps;           // of the build: a field's history has max_steps + 1 rows
    const unsigned short* field;
    const u64* hist;         // [n_fields][max_steps + 1][nz * ny * W]
    const int* last;         // [n_fields]: the last row the build wrote
};
struct dspmap_reach_point;
#define REACH_LDS_BYTES (160 * 1024 - 256)   // what a workgroup's two sets may take of the CU's 160 KiB (the rest: the step flags)
void reach_init_device();   // per device, once (dspmap_init_device)
void launch_reach(const LaunchCtx& c, const ReachArgs& a, const struct dspmap_reach_point* src, u64* hist, int* last);
void launch_reach_timeline_paths(const LaunchCtx& c, const ReachTimelinePathArgs& a, int n, const struct dspmap_reach_point* start, int* steps_out,
                                 int* cells_out);
// weighted: the descent by the weight of the cell left (cost paths, a.weight set); otherwise the steepest descent by 1 (reach paths)
void launch_field_paths(const LaunchCtx& c, const FieldPathArgs& a, bool weighted, int n, const struct dspmap_reach_point* start, int* steps_out, int* cells_out);
// clearance-weighted cost-to-go fields: a bucketed wavefront through one layer of the cast grid, one workgroup per field (dspmap_cost.hip;
// semantics in include/dspmap.h, dspmap_build_cost_fields)
#define COST_MAX_BANDS 4    // == DSPMAP_COST_MAX_BANDS
#define COST_MAX_WEIGHT 8   // == DSPMAP_COST_MAX_WEIGHT
#define COST_SET_COUNT 11   // sets of nz * ny * W words a field's scratch holds: 8 grown level sets, 2 level sets, settled
struct CostWeightArgs {
    int n_bands;
    float clearance[COST_MAX_BANDS];
    int penalty[COST_MAX_BANDS];
    const u64* bits;         // [nz][ny][W] the build's layer of the cast grid
    const float* dist;       // [V] the build's layer of the distance field; not read when n_bands == 0
    unsigned char* weight;   // [V] 0 blocked, else w
    u64* wk;                 // [COST_MAX_WEIGHT][nz][ny][W] the cells of weight k, k = 1 ..
    int* occ;                // bit k: weight k occurs (zeroed on the stream before the launch)
};
struct CostArgs {
    SampleOrigin org;
    int max_cost;
    int n_fields, n_src;
    const u64* wk;       // as CostWeightArgs
    const int* occ;
    unsigned short* field;   // [n_fields][V], preset to DSPMAP_COST_UNREACHED
    u64* sets;           // [n_fields][COST_SET_COUNT][nz * ny * W] device scratch
};
void launch_cost_weights(const LaunchCtx& c, const CostWeightArgs& a);
void launch_cost_wave(const LaunchCtx& c, const CostArgs& a, const struct dspmap_reach_point* src);   // (the paths: launch_field_paths)
// cell paths shortened to line-of-sight waypoints, one wave per path (dspmap_shorten.hip; semantics in include/dspmap.h, dspmap_shorten_paths)
struct ShortenArgs {
    float cx, cy, cz;    // as QueryArgs: dspmap_voxel_center
    int timed;           // t_start >= 0 and T > 0: cell j has the time of step max(steps - j, 0); otherwise every vertex has time -1
    float t_start, step_seconds;
    int max_len, window, max_seg;
    const u64* bits;     // [L][nz][ny][W]
};
struct dspmap_path_info;
void launch_shorten(const LaunchCtx& c, const ShortenArgs& a, int n, const int* steps, const int* cells, struct dspmap_path_info* info,
                    struct dspmap_segment* seg, int* end);
// occupancy forecast at caller-chosen times from the live particle set (dspmap_forecast.hip; semantics in include/dspmap.h, dspmap_build_forecast)
#define FORECAST_MAX_TIMES 64   // == DSPMAP_FORECAST_MAX_TIMES
struct ForecastArgs {
    int n;               // layers
    float t[FORECAST_MAX_TIMES];   // their times, strictly ascending
    u64* dyn;            // [n][v_loc] quanta of the moving particles, storage order (zeroed on the stream before the sweep)
    u64* stat;           // [v_loc] quanta of the static particles: the same in every layer (zeroed likewise: the sweep leaves empty tiles early)
    float* out;          // [n][V] the layers in the reference's voxel order
};
void launch_forecast(const LaunchCtx& c, const ForecastArgs& a);
struct ForecastQueryArgs {
    SampleOrigin org;
    int lerp;            // DSPMAP_FORECAST_LERP
    float outside;       // what a point outside the map or a NaN sample reads
    int n;
    float t[FORECAST_MAX_TIMES];
    const float* field;  // [n][V]
};
void launch_forecast_query(const LaunchCtx& c, const ForecastQueryArgs& a, int n, const float4* q, float* out);
// known-space layer (dspmap_known.hip; semantics in include/dspmap.h, dspmap_known_integrate).  These launchers take the dimensions and the
// stream, not a LaunchCtx: nothing of the frame's scratch or of its launch decisions is involved
struct KnownArgs {
    unsigned* stamp;     // [nz][ny][nx] SLOTS: lattice cell k of an axis lives in slot k mod n; 0 = never, else the update counter of the last frame that saw it
    int bx, by, bz;      // the slot of map voxel 0 per axis: k0 mod n, in [0, n)
    float ox, oy, oz;    // centre of the lattice cell behind voxel (0, 0, 0) relative to the sensor
    float max_range;     // the caller's sensor range (+inf: none)
    float occl_margin;   // FilterParams::occl_margin
    unsigned now;        // the handle's update counter
};
void launch_known_integrate(const MapDims& d, const DevState& s, hipStream_t stream, const KnownArgs& a, int n_cu);
void launch_known_clear(const MapDims& d, hipStream_t stream, unsigned* stamp, const int slot0[3], const int count[3]);   // per axis: slots [slot0, slot0 + count) mod n
void launch_known_ages(const MapDims& d, hipStream_t stream, const KnownArgs& a, int* out);   // [V] ages, the reference's voxel order
void launch_known_query(const MapDims& d, hipStream_t stream, const KnownArgs& a, const SampleOrigin& org, int n, const float4* q, int* out);
void launch_known_count(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, u64* sums);   // sums[2], zeroed by the caller
void launch_known_mask(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, int L, u64* bits);
// scores of candidate viewpoints (dspmap_view.hip; semantics in include/dspmap.h, dspmap_score_views).  As the known-space launchers: the
// dimensions and the stream, no LaunchCtx
struct ViewArgs {
    SampleOrigin org;
    const u64* bits;     // [L][nz][ny][W] the cast grid
    KnownArgs kn;        // the synchronised known-space layer (max_range is not read: every view brings its own)
    int max_age;         // a seen cell is unknown iff its age is -1 or > max_age
    float cx, cy, cz;    // as QueryArgs: dspmap_voxel_center
    const float* dirs0;  // [np][3] unrotated central direction of every pyramid
    float reach;         // fl(res * (float)(nx + ny + nz)): no ray is longer
};
static_assert(offsetof(QueryArgs, org) == 0 && offsetof(DistQueryArgs, org) == 0 && offsetof(CastArgs, org) == 0 && offsetof(BoxArgs, org) == 0 &&
                  offsetof(ReachArgs, org) == 0 && offsetof(FieldPathArgs, org) == 0 && offsetof(ReachTimelinePathArgs, org) == 0 &&
                  offsetof(CostArgs, org) == 0 && offsetof(ForecastQueryArgs, org) == 0 && offsetof(ViewArgs, org) == 0 &&
                  offsetof(NearQueryArgs, org) == 0,
              "every argument block that takes samples starts with their SampleOrigin");
struct dspmap_view;
struct dspmap_view_score;
int view_chunks(const MapDims& d, int n, int n_cu, int forced);   // workgroups per view for a batch of n (forced > 0: that many, capped)
// out [n] zeroed by the caller; dbg_words ([nz][ny][W], zeroed) / dbg_ml ([np]): the seen set and the farthest returns (n == 1), or nullptr
void launch_view_score(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, int n, int chunks, const struct dspmap_view* views,
                       struct dspmap_view_score* out, u64* dbg_words, float* dbg_ml);
// out: planes_h [(np_h + 1) * 3], planes_v [(np_v + 1) * 3], dirs [np * 3] of attitude q, consecutively
void launch_view_rays(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, const float q[4], float* out);
// joint gain of views (dspmap_viewsel.hip; semantics in include/dspmap.h, dspmap_score_view_sets).  lw: the words of a layer, nz * ny * W
// launch_view_score, and every view's seen set into masks [n][lw], CLEARED by the caller (only non-zero words are stored)
void launch_view_masks(const MapDims& d, const DevState& s, hipStream_t stream, const ViewArgs& a, int n, int chunks, const struct dspmap_view* views,
                       struct dspmap_view_score* out, u64* masks);
struct dspmap_view_set_score;
struct dspmap_view_pick;
int viewsel_chunks(int lw, int n, int n_cu, int forced);   // workgroups per set / candidate for a batch of n (forced > 0: that many, capped)
void launch_viewsel_unknown(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, u64* unk);   // unk [lw]: bit = age -1 or > max_age
// out [n_sets] zeroed by the caller; avail (NULL, or [lw] with n_sets == 1): unk & ~union
void launch_viewsel_sets(hipStream_t stream, int lw, int n_sets, int set_size, int chunks, const u64* masks, const u64* unk,
                         const struct dspmap_view_score* scores, struct dspmap_view_set_score* out, u64* avail);
// round r of the greedy selection among views [n_fixed, n_fixed + n_cand): gain (zero on entry, zero on exit), picks[r], avail &= ~picked mask
void launch_viewsel_round(hipStream_t stream, int lw, int n_fixed, int n_cand, int chunks, int r, int min_gain, const u64* masks, u64* avail,
                          int* gain, const struct dspmap_view_set_score* fixed, struct dspmap_view_pick* picks);
// frontier cells and blocks (dspmap_frontier.hip; semantics in include/dspmap.h, dspmap_build_frontiers).  As the known-space launchers: the
// dimensions and the stream, no LaunchCtx
struct dspmap_frontier_block;
#define FR_TILE 256   // items (grid words / blocks) per tile of the ordered compaction: one workgroup, one item per thread
inline int frontier_tiles(long long n) { return (int)((n + FR_TILE - 1) / FR_TILE); }
struct FrontierArgs {
    KnownArgs kn;        // the synchronised known-space layer
    const u64* bits;     // [nz][ny][W] the SELECTED layer of the cast grid
    int max_age, min_unknown, block;
    int nbx, nby, nb;    // blocks along x, along y, and in all
    u64* grid;           // out [nz][ny][W] frontier bits
    int* cells;          // out [n_cells <= V] ascending voxel indices
    struct dspmap_frontier_block* dense;    // [nb] the blocks' accumulators, zeroed by the caller (.block is not used)
    struct dspmap_frontier_block* blocks;   // out [n_blocks <= nb] the non-empty ones, ascending
    int* item_free;      // scratch [nz * ny * W] free cells per grid word
    int* tile_sum;       // scratch [tiles of the words + tiles of the blocks] per-tile sums, then exclusive bases
    int* tile_free;      // scratch [tiles of the words]
    long long* counts;   // out {n_cells, n_blocks, n_free}
    int merge;           // DSPMAP_P_FRONTIER_MERGE: block sums per (wave, block) instead of per cell
};
void launch_frontiers(const MapDims& d, hipStream_t stream, const FrontierArgs& a);
// objects: the connected components of one layer of the cast grid (dspmap_objects.hip; semantics in include/dspmap.h, dspmap_build_objects)
struct dspmap_object;
#define OBJ_COUNTS 4   // long longs of the counts buffer: {n_objects, n_components, n_occupied} and the fault word
struct ObjectArgs {
    const u64* bits;     // [nz][ny][W] the SELECTED layer of the cast grid
    int conn;            // 6 or 26
    int min_cells, max_objects;
    int* parent;         // [V] union-find labels, -1 for a clear bit; after the flattening the root (= smallest voxel index) of the cell's component
    int* root_val;       // [V] zeroed by the caller: per root its cell count, then its ordinal (-1 below min_cells)
    int* labels;         // out [V] the label grid
    struct dspmap_object* objects;   // out [min(max_objects, V)]
    int* tile_sum;       // scratch [tiles of V]
    long long* counts;   // out [OBJ_COUNTS], zeroed by the caller
};
void launch_objects(const LaunchCtx& c, const ObjectArgs& a);
void launch_objects_query(const LaunchCtx& c, const int* labels, const SampleOrigin& org, int n, const float4* q, int* out);
// tracks: the objects of consecutive builds associated by voxel overlap (dspmap_track.hip; semantics in include/dspmap.h, dspmap_track_update)
struct dspmap_track;
#define TRK_COUNTS 6     // long longs of the counts: {n_tracks, n_matched, n_born, n_ended, n_pairs, next_id}
#define TRK_FAULT 6      // ... behind them: 0, or 1 when the pair table was full
#define TRK_KEPT 7       // ... and two words that live through the updates: the records the stored previous state holds (K_prev)
#define TRK_NEXT 8       //     and the next fresh id
#define TRK_WORDS 9
#define TRK_ORD_BITS 20  // a pair's key is ((j << 20 | o) + 1): ordinals stay below DSPMAP_OBJECTS_MAX = 2^20
struct TrackArgs {
    const int* labels;                     // [V] the label grid, the records and the counts of the valid build of objects
    const struct dspmap_object* objects;
    const long long* obj_counts;
    int max_objects;                       // ... and its max_objects: K_now = min(obj_counts[0], max_objects)
    const int* p_labels;                   // [V] the tracker's copies from the previous update; K_prev = counts[TRK_KEPT]
    const struct dspmap_object* p_objects; // [cap]
    const struct dspmap_track* p_tracks;   // [cap] the previous tracks
    struct dspmap_track* tracks;           // out [cap]
    int4* shift;                           // scratch [cap]: shift_j, per previous track
    u64* best_prev; u64* best_now;         // scratch [cap] each, zeroed by the caller unless fresh
    u64* keys; int* vals;                  // the pair table [slots], zeroed by the caller unless fresh
    int slots;                             // a power of two
    int* tile_sum;                         // scratch [tiles of cap]
    long long* counts;                     // [TRK_WORDS], the first TRK_FAULT + 1 zeroed by the caller
    int cap;                               // records every per-record array holds
    int fresh;                             // nothing is associated: no previous state, or the window moved by a whole map
    int dk0[3];                            // k0_now - k0_prev
    int min_overlap, max_shift, per_cell, seq;
    float dt;
};
void launch_track(const LaunchCtx& c, const TrackArgs& a);
// state helpers
void launch_seed_uniform(const LaunchCtx& c, int per_voxel, float weight, unsigned seed, float vmax);
void launch_import(const LaunchCtx& c, int n, const int* voxel_dev, const int* slot_dev, const float* rec8_dev, int* n_failed_dev);
void launch_export(const LaunchCtx& c, int* voxel_out, int* slot_out, float* rec8_out, int* count_dev, int cap);
void launch_add_random(const LaunchCtx& c, int n, float weight, int* slot_of_tmp /* [n] device scratch */);
