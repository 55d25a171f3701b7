/*
 * dspmap.h -- C ABI of libdspmap_hip.so: the MI355X-native particle-based
 * dynamic occupancy mapper (hand-written HIP kernels for gfx950).
 *
 * This is the drop-in boundary for the per-frame loop of g-ch/DSP-map's
 * include/dsp_dynamic.h (class DSPMap).  Every entry point names the reference
 * interface it replaces (file:line relative to the reference tree).  Plain
 * pointers and sizes only; no C++/torch types cross this boundary.  The C++
 * class surface (`class DSPMap`, include/dsp_dynamic.h in THIS repo) and the
 * Python/ctypes binding (dsp-map_amd/capi.py) are thin forwards to it; the
 * binding a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - All functions return DSPMAP_OK (1) on success unless stated otherwise;
 *    0 = "frame rejected, state unchanged" for update (as the reference's
 *    `return 0`, dsp_dynamic.h:193-208); negative = error, text via
 *    dspmap_last_error().  Nothing throws.  There is NO CPU fallback: if no
 *    HIP device is usable every compute entry point fails with DSPMAP_E_DEVICE.
 *  - `host` pointers are caller-owned host memory, never retained past return.
 *    `dev` pointers are device memory on the handle's device.
 *  - One frame in flight per handle; a handle is not re-entrant (the reference
 *    is not either: function statics + file-scope state, dsp_dynamic.h:116-140,187-190).
 *  - Voxel indexing, slot capacity, pyramid (angular bin) layout and all
 *    constants follow the reference (dsp_dynamic.h:38-70).
 */
#ifndef DSPMAP_H
#define DSPMAP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSPMAP_OK 1
#define DSPMAP_REJECTED 0
#define DSPMAP_E_ARG (-1)
#define DSPMAP_E_DEVICE (-2)
#define DSPMAP_E_STATE (-3)

#define DSPMAP_MAX_PRED_TIMES 16

typedef struct dspmap dspmap_t;

/* Run-time replacement of the reference's compile-time macros
 * (dsp_dynamic.h:38-50) plus what a multi-GPU shard needs. */
typedef struct dspmap_config {
    int nx, ny, nz;             /* MAP_LENGTH/WIDTH/HEIGHT_VOXEL_NUM  :38-40 */
    float voxel_resolution;     /* VOXEL_RESOLUTION                   :41 */
    int angle_resolution;       /* ANGLE_RESOLUTION, degrees          :42 */
    int max_particle_num_voxel; /* MAX_PARTICLE_NUM_VOXEL             :43 */
    int half_fov_h, half_fov_v; /* :49-50, degrees */
    int prediction_times;       /* PREDICTION_TIMES                   :46 */
    float prediction_future_time[DSPMAP_MAX_PRED_TIMES]; /* :47 */
    /* Z-slab owned by this handle: voxel layers [z_lo, z_hi) of the global
     * grid (voxel index is z-major, :1081).  z_lo == z_hi == 0 means all. */
    int z_lo, z_hi;
    int device;                 /* HIP device ordinal, -1 = current device */
    int gaussian_table_size;    /* GAUSSIAN_RANDOMS_NUM :72 (10,000,000); 0 = default */
    unsigned seed;              /* table/rand seed; 0 = time(NULL) like :586,1151 */
    /* the reference's two other headers as run-time parameters of the same kernels; 0 = dsp_dynamic.h's value */
    int pyramid_neighbor_n;     /* PYRAMID_NEIGHBOR_N (dsp_dynamic_multiple_neighbors.h:43: 2 -> 5x5 neighbourhood); default 1 */
    int safe_particle_factor;   /* SAFE_PARTICLE_NUM_VOXEL / MAX_PARTICLE_NUM_VOXEL: default 2 (:65); dsp_static.h:63 uses 5 */
    int static_model;           /* 1 = dsp_static.h: velocities forced to zero in prediction, every birth source static */
} dspmap_config;

/* Birth-source point = one entry of the reference's input_cloud_with_velocity
 * (pcl::PointXYZINormal, dsp_dynamic.h:134,1510-1539): world-frame xyz,
 * normal = estimated velocity (-10000 when the cluster is unmatched, :104-106),
 * intensity = cluster tag (0 = static / ground). */
typedef struct dspmap_vpoint {
    float x, y, z;
    float nx, ny, nz;
    float intensity;
} dspmap_vpoint;

/* Per-frame device counters (the reference computes similar counters and
 * never prints them, dsp_dynamic.h:629-632,926-927). */
typedef struct dspmap_counters {
    int n_points_in;       /* points handed to update() */
    int n_valid;           /* valid_points :286 (in FOV, incl. overflowed) */
    int n_obs;             /* stored observations (<= 99 per pyramid, :279-284) */
    int n_live_in;         /* live particles entering prediction */
    int n_moved;           /* particles that changed voxel */
    int n_out_of_map;      /* removed: left the map :688 */
    int n_voxel_full;      /* removed: destination voxel full (-1, :1227) */
    int n_pyramid_full;    /* removed: pyramid list full (-2, :1256) */
    int n_fov;             /* particles registered in pyramids after prediction */
    int n_born;            /* newborn particles inserted :911 */
    int n_born_dropped;    /* newborn dropped: voxel full :1198 */
    int n_live_out;        /* live particles after resampling */
    int n_exported_up, n_exported_down; /* multi-GPU: left the slab through z_hi / z_lo */
    int n_reslotted;       /* voxels whose arrivals were re-slotted because a full pyramid list turned a particle away (:1256-1259) */
    int n_overflow_inexact;/* diagnostics: arrivals / voxels that pass could not treat exactly (destination voxel full AND list full) */
    float newborn_weight;  /* updated_weight_new_born :805 */
    float update_ms;       /* device time of the last TIMED update (HIP events): every frame of the host-staged path, every 32nd frame
                              of dspmap_update_device's replayed graph (an event record between two replays costs ~5 us) */
} dspmap_counters;

enum dspmap_param {
    DSPMAP_P_POSITION_STDDEV = 1,   /* setPredictionVariance arg 1   :355 */
    DSPMAP_P_VELOCITY_STDDEV = 2,   /* setPredictionVariance arg 2   :355 */
    DSPMAP_P_OBSERVATION_STDDEV = 3,/* setObservationStdDev          :362 */
    DSPMAP_P_NEWBORN_WEIGHT = 4,    /* setNewBornParticleWeight      :366 */
    DSPMAP_P_NEWBORN_NUMBER = 5,    /* setNewBornParticleNumberofEachPoint :370 */
    DSPMAP_P_VOXEL_FILTER_RES = 6,  /* setOriginalVoxelFilterResolution :380 */
    DSPMAP_P_KAPPA = 7,             /* kappa :157 */
    DSPMAP_P_DETECTION = 8,         /* P_detection :158 */
    DSPMAP_P_VELOCITY_ESTIMATOR = 9,/* velocityEstimationThread (:297,1377-1544) inside update(): 2 = on the device, a side branch of the
                                       captured frame (dspmap_velest.hip; the drop-in class's default); 1 = host stage overlapped
                                       with the kernels (velocity_estimator.cpp); 0 = births use the caller's cloud, or tag every
                                       point in view as a static source */
    DSPMAP_P_REGENERATE_TABLES = 10,/* 1 = setPredictionVariance regenerates the Gaussian tables (:359) */
    DSPMAP_P_USE_GRAPH = 11,        /* how dspmap_update / dspmap_update_device queue a frame.  2 = its kernels as plain launches, parameter block through the pinned
                                       ring: no graph boundary between two frames (8.7 us on this runtime: 66x66x40 0.151 -> 0.142 ms) but twelve launches of host
                                       time per frame (2.5 - 3 us each; ~100 us per frame once the caller runs hundreds of launches ahead of the device).  3 = the
                                       frame replayed as a captured HIP graph wherever it can be captured (one launch, ~18 us of host time per frame).  1 (default) =
                                       2 for the device-resident frames (dspmap_update_device, dspmap_update_depth*) of maps with fewer than 8 192 tiles of 64 voxels
                                       whose chain is one stream's kernels (estimator on its own queue, or none; no split placement): A -4.4 %, B -5.8 % against
                                       the graph in process -- and 3 for everything else: larger maps (132x132x60 filled by the depth stream -2 % with overlapping
                                       ranges, 264x264x80 -0.8 %, saturated ones +0.4 % or never eligible) and every host-pointer dspmap_update, whose caller
                                       would pay the launches (measured host-bound at 4 800 frames/s).  0 = plain launches with a copied parameter block (rounds
                                       1-2; what stage profiling uses).  Same result whichever way, bit for bit */
    DSPMAP_P_OCCLUSION_MARGIN = 12, /* obstacle_thickness_for_occlusion :70 (0.3 m); the reference's two other headers use VOXEL_RESOLUTION */
    DSPMAP_P_UPDATE_TIME = 14,      /* read-only: update_time, the sum of the accepted frames' delt_t (:634) */
    DSPMAP_P_UPDATE_COUNTER = 15,   /* read-only: update_counter, the number of predictions run (:635) */
    DSPMAP_P_PLACE_SPLIT_TILES = 16,/* maps with at least this many 64-voxel tiles (default 8192) give the voxel-changing particles of the tiles
                                       that cannot see the sensor's field of view their slots on a side stream, beside the weight update
                                       (same result; a scheduling knob: 1 = always, a huge value = never; not while the handle sweeps the map
                                       as a sparse one -- most tiles empty, DSPMAP_P_SPARSE_SWEEP -- unless the value is 1; the environment
                                       variable DSPMAP_PLACE_SPLIT_TILES presets it at dspmap_create) */
    DSPMAP_P_FAST_DIVISION = 17,    /* read: 1 if (p + half) / VOXEL_RESOLUTION (:1062-1088) is computed as reciprocal + two FMAs -- only after a
                                       kernel has compared that quotient with the IEEE division, bit for bit, for this resolution
                                       (device initialisation); write 0: force the IEEE division (same results by construction) */
    DSPMAP_P_SPARSE_SWEEP = 18,     /* which variant of the prediction sweep runs: -1 (default) the handle decides from a running estimate of how
                                       many 64-voxel tiles hold particles (most empty: empty tiles are left after one scalar load), 0 / 1 force
                                       one (same result either way; read: the variant of the last frame) */
    DSPMAP_P_ROLLOUT_INLINE = 19,   /* maps small enough for the four-waves-per-tile resampler: 1 = its tiles add their moving particles' future
                                       status themselves (one float atomic per particle and horizon; no k_rollout launch), 0 = k_rollout's LDS
                                       windows, -1 (default) the handle decides from the number of tiles with hundreds of moving particles; larger
                                       maps: 1 = k_rollout without windows, 0 = with them.  The future status is accumulated in fixed point, every
                                       particle adds the same integer on every path: the SAME result bit for bit (read: the last frame's choice) */
    DSPMAP_P_RESAMPLE_WG_TILES = 20,/* one-occupancy-word maps with FEWER 64-voxel tiles than this (default 8192) -- and larger ones while the handle takes
                                       them for sparse (most tiles empty, DSPMAP_P_SPARSE_SWEEP) -- run the four-waves-per-tile variant of the
                                       resampling stage, the others the one-wave-per-tile variant (same result slot for slot; a scheduling knob: 0 =
                                       never, a huge value = whenever the map qualifies; the environment variable DSPMAP_RESAMPLE_WG_TILES presets it) */
    DSPMAP_P_SWEEP_ALTERNATE = 21,  /* direction of the three sweeps over the map's 64-voxel tiles.  A large map's live rows are several times the 256 MB
                                       Infinity Cache, so a sweep that starts where its predecessor ENDED finds its first tiles there instead of in HBM:
                                       2 (default) = prediction upwards, placement of the voxel-changing particles downwards, resampling downwards (and
                                       the next frame's prediction starts where it ended); 0 = resampling upwards; 1 = all three flip from frame to frame
                                       (two captured graphs); -1 = 1 on maps of at least 4096 tiles.  132x132x60 saturated: placement -15 %, frame -3 %.
                                       Same result in every mode: no stage depends on the order in which the tiles are visited */
    DSPMAP_P_STATIC_TILE_SKIP = 22, /* 1 (default): a 64-voxel tile whose live particles all have velocity (0, 0) is swept without its velocity rows, keeps
                                       its velocity cells zeroed, and a static particle that arrives there is placed without a velocity store (the
                                       reference never gives a static particle a velocity, :653); 0 = every tile is treated as if something moved in it.
                                       Same result either way, bit for bit (the diagnostic the differential GPU test switches) */
    DSPMAP_P_HOST_CLOUD_DIRECT = 23,/* 1 (default): dspmap_update (the host-pointer update() of the reference, :181) copies the caller's cloud into a
                                       slot of a pinned, device-mapped ring and the captured frame's first kernel reads it over the bus: the frame is
                                       ONE graph launch (needs DSPMAP_P_USE_GRAPH and the device velocity estimator); 0 = pinned staging + one H2D
                                       copy + an event in front of the graph (rounds 1-4).  Same result either way */
    /* 24: early registration of the voxel-changing particles by the prediction sweep (round 5) -- measured slower on the maps it was
       built for and removed in round 6 (LOG.md); the value is not reused */
    DSPMAP_P_ESTIMATOR_QUEUE = 25,  /* captured frames with the device velocity estimator (DSPMAP_P_VELOCITY_ESTIMATOR = 2) on maps that do not split their
                                       placement: 1 (default) = the estimator's kernels are launched on a stream of their own, BEFORE the frame, and meet it
                                       through two words in device memory: the estimator makes its own picture of the view from the frame's slot of the
                                       parameter ring (k_ve_view) and waits only for "the PREVIOUS frame's birth stage has ended" (published by that frame's
                                       resampling kernel: the rand() cursor and the birth buffers are the estimator's from then on); the frame's first birth
                                       kernel waits for "the birth cloud is complete" (published by the estimator's last kernel behind a release fence).  The
                                       reference's helper thread (:297,311) without a fork / join inside the graph, which costs ~8 us of a 147-us frame on
                                       this runtime (tools/micro/fork_join.hip).  Every wait is for work submitted earlier and is bounded (200 ms): a wait
                                       that gives up calls the frame's birth stage off, the next call fails once and the handle goes on with 0.  The stream
                                       is tested not to share the main stream's hardware queue; if none is found the handle keeps 0's path
                                       (dspmap_debug_estimator_path).  0 = a forked branch of the captured graph (rounds 2-5).  Same result either way.
                                       WHAT THE WAIT CANNOT COVER: the estimator's matching is the sequential Hungarian algorithm in one wavefront; a frame
                                       in which every new cluster is gated against every old one (a scene change, everything moved 1.5 m or more) or whose
                                       cluster count jumps takes N (N + 1) / 2 steps for N = max(new, old) possibly-dynamic clusters.  Measured on the
                                       MI355X (tools/velest_scaling.py): 17 ms at N = 128, 127 ms at N = 300, i.e. half the wait from about
                                       270 clusters and the whole wait from about 340 (extrapolated: 0.7 s at 512, 8.5 s at the capacity of 1 228).
                                       Such a frame is computed WITHOUT its birth stage, the next call returns DSPMAP_E_DEVICE once, and the handle goes on
                                       with 0.  A caller whose scenes can hold more than ~250 clusters of 5+ points sets 0 here (no wait, the frame simply
                                       takes as long as the matching) or DSPMAP_P_VELOCITY_ESTIMATOR = 1.  Frames whose clusters find their predecessors
                                       take N steps: 0.4 ms at 128, 1.2 ms at 300 */
    DSPMAP_P_FRAME_BRANCHES = 26,   /* whole frames of dense large maps run as TWO BRANCHES (round 6): the part of the map the sensor can see this frame -- grown by
                                       the reach of a newborn (:871-873) and by the frame's largest displacement (:665-667) -- goes through prediction,
                                       placement, mapUpdate, births and resampling on the main stream, the rest of the map (most of it: prediction,
                                       placement, resampling only -- the bandwidth-bound sweeps) beside it on a forked branch.  -1 (default) = the maps that
                                       would split their placement (DSPMAP_P_PLACE_SPLIT_TILES), 0 = never (the serial frame of rounds 1-5), 1 = whenever
                                       the frame allows it (any size; what the differential tests force).  Same result slot for slot.  The environment
                                       variable DSPMAP_FRAME_BRANCHES presets it */
    DSPMAP_P_TILING = 27,           /* which 64 voxels share a tile of the particle store (one wave, one lane per voxel): 0 = 64 consecutive voxel indices (a run along
                                       x; rounds 1-5), 1 = a cube of 4 x 4 x 4 voxels, -1 (default) = cubes on unsharded maps large enough for the two-branch
                                       frame, runs otherwise.  A run that points away from the sensor is cut by the field of view almost wherever it lies (58 %
                                       of the 132x132x60 map's runs have a view, 19 % of its cubes).  Settable only before the handle's first use (read: the
                                       order in use); sharded handles (Z-slabs) keep index order.  Results, state records and sweep order are the reference's
                                       whatever the storage: the same result slot for slot.  The environment variable DSPMAP_TILING presets it */
    DSPMAP_P_SIDE_PLACEMENT = 28,   /* frames that split their placement (DSPMAP_P_PLACE_SPLIT_TILES): value = 16 * fork + footprint.  fork: where the launch that
                                       places the arrivals of the tiles without a view leaves the main chain -- 0 behind the list preparation (rounds 3-5), 1
                                       (default) behind the placement of the tiles with a view, 2 behind the prediction; footprint: its workgroups per compute
                                       unit (1 .. 15, default 3); a negative value restores the default (19).  Measured on identical maps in one process
                                       (tools/ab_maps.py): 132x132x60 saturated 19 against 3: -2.9 %, 35: +8 %; 264x264x80 saturated: -1.4 %.  A scheduling knob:
                                       same result slot for slot */
    DSPMAP_P_RESAMPLE_SPLIT = 29,   /* frames that split their placement on cube storage, with a birth cloud made on the device from the frame's own view
                                       (DSPMAP_P_VELOCITY_ESTIMATOR 2, or every point in view a static source): 1 = the resampling stage (:924-1057) runs as two
                                       launches -- the tiles no newborn of this frame can reach (outside the field of view grown by the position table's
                                       largest value) on the side stream, right behind the placement it carries, BESIDE the weight update and the birth
                                       stage of the main chain; the others behind the births; the rollout behind both.  A frame with an empty view (stale
                                       birth cloud, :1379-1381) resamples every tile behind the births.  0 = one launch behind the births.  Same result
                                       slot for slot.  The environment variable DSPMAP_RESAMPLE_SPLIT presets it */
    DSPMAP_P_TILE_BITMAPS = 30,     /* whole frames of an unsharded map the handle sweeps as a sparse one (most 64-voxel tiles empty, DSPMAP_P_SPARSE_SWEEP): 1
                                       (default) = the three sweeps (prediction, placement, resampling) learn that a tile has nothing for them from one BIT per
                                       tile -- tables of a few kB that stay in the scalar cache, rebuilt from the per-tile flags by the frame's first kernel
                                       and extended by whoever puts the first particle into an empty tile -- instead of from the tile's own words in
                                       memory: an empty tile's workgroup leaves as fast as the next one can be started (264x264x80 filled by the depth
                                       stream: 87 120 tiles, ~12 k with particles); 0 = every workgroup loads its tile's flags (rounds 3-5).  Same result */
    DSPMAP_P_VIEW_CHUNKS = 31,      /* dspmap_score_views*: workgroups per view.  0 (default) = the handle spreads a batch over the device: about four
                                       workgroups per compute unit in all, at most 64 per view and never more than the map has rows for; 1 .. 64 = that
                                       many (capped likewise).  The scores are integer counts and do not depend on it */
    DSPMAP_P_FRONTIER_MERGE = 32,   /* dspmap_build_frontiers: 1 (default) = the frontier lanes of a wave that fall into one block are summed with
                                       ballots and popcounts and added to the block's record by one lane (five integer atomics per wave and block);
                                       0 = every frontier lane adds its own cell (five per cell).  For measurement: integer sums, the same result */
    DSPMAP_P_PAIR_PREPARE = 33,     /* whole frames (dspmap_update_device, dspmap_update with the device estimator) of an unsharded map whose weight update evaluates
                                       every pair (dspmap_debug_weight_variant 1) and that neither split their placement nor run as two branches: 0 (default) = the
                                       pair kernels map their work items themselves and read the pyramid lists as they were registered -- no k_pyr_prepare launch --
                                       until a frame finds a list past SAFE_PARTICLE_NUM_PYRAMID: that frame sorts and cuts inside its Ck launch, and the handle
                                       prepares its lists from the next frames on, until dspmap_clear_state / dspmap_load_checkpoint; 1 = always k_pyr_prepare;
                                       2 = self-mapped wherever legal, overfull lists or not (for tests).  Same result bit for bit; dspmap_debug_pair_path */
    DSPMAP_P_PAIR_CULL_SIGMAS = 13  /* mapUpdate evaluates a (particle, observation) pair only if their ranges differ by at most this many
                                       sigma_ob (default 9: the dropped terms are < 1e-19 and zero on the fixed-point Ck grid);
                                       a huge value evaluates every pair of the neighbourhood like the reference's loops */
};

/* ---- lifecycle: DSPMap::DSPMap / ~DSPMap  dsp_dynamic.h:145-179 ---- */
void dspmap_default_config(dspmap_config* cfg);          /* the reference's shipped macro values */
dspmap_t* dspmap_create(const dspmap_config* cfg);        /* no HIP call: safe during static init (src/map_sim_example.cpp:39) */
void dspmap_destroy(dspmap_t* m);
int dspmap_init_device(dspmap_t* m);                      /* allocate device state now (otherwise lazily on first use) */
const char* dspmap_last_error(const dspmap_t* m);
int dspmap_sync(dspmap_t* m);                             /* wait for all queued work of this handle */
int dspmap_set_stream(dspmap_t* m, void* hip_stream);     /* run on a caller-owned hipStream_t (e.g. torch's) */
void* dspmap_get_stream(const dspmap_t* m);               /* the hipStream_t the handle queues on (NULL before its device state exists
                                                             unless one was set): what a caller orders its own streams / allocator with */

/* ---- setters: dsp_dynamic.h:355-382 ---- */
int dspmap_set_param(dspmap_t* m, int key, double value);
double dspmap_get_param(const dspmap_t* m, int key);

/* ---- randomness.  The reference pre-draws two N(0,sigma) tables
 * (dsp_dynamic.h:138-139,1150-1160) and uses libc rand() for uniform
 * velocities (:1551-1553).  Tables can be injected so that runs can be
 * compared with another implementation fed the same tables. ---- */
int dspmap_set_gaussian_tables(dspmap_t* m, const float* p_tab_host, const float* v_tab_host, int n);
int dspmap_set_rand_table(dspmap_t* m, const int* rand_ints_host, int n); /* values in [0, RAND_MAX] */
int dspmap_set_cursors(dspmap_t* m, int p_cursor, int v_cursor, int r_cursor);
int dspmap_get_cursors(dspmap_t* m, int* p_cursor, int* v_cursor, int* r_cursor);

/* ---- the frame: DSPMap::update  dsp_dynamic.h:181-353 ----
 * Same arguments and the same 1 / 0 contract (0 = invalid quaternion or
 * |dp| > 10 m or dt outside [0,10] s; state and the "last pose" untouched). */
int dspmap_update(dspmap_t* m, int point_cloud_num, int size_of_one_point, const float* point_cloud_host,
                  float sensor_px, float sensor_py, float sensor_pz, double time_stamp_second,
                  float qw, float qx, float qy, float qz);

/* Same frame with inputs already resident in HBM: `points_dev` = n x 3 floats
 * (sensor frame, packed xyz); `birth_dev`/n_birth = the birth-source cloud
 * (what the velocity estimator would output) or NULL/0 = every in-FOV point is
 * a static source (zero velocity tag) -- unless DSPMAP_P_VELOCITY_ESTIMATOR is set:
 * 2 = the device estimator tags the cloud inside the captured frame (still
 * asynchronous); 1 = the cloud makes one round trip to the host estimator (D2H of
 * <= 60 kB, clustering + matching while the prediction and weight kernels run, H2D
 * of the tagged cloud).  Asynchronous otherwise: returns after enqueue. */
int dspmap_update_device(dspmap_t* m, int n_points, const float* points_dev, int n_birth,
                         const dspmap_vpoint* birth_dev, const float sensor_pos[3],
                         double time_stamp_second, const float quat_wxyz[4]);

/* Supply the birth-source cloud used by the next dspmap_update /
 * dspmap_stage_birth when the velocity estimator is off (what the reference's
 * velocityEstimationThread leaves in input_cloud_with_velocity, :134). */
int dspmap_set_birth_cloud(dspmap_t* m, const dspmap_vpoint* pts_host, int n);
/* getKMClusterResult :441-445 : the birth-source cloud of the last frame */
int dspmap_get_birth_cloud(dspmap_t* m, dspmap_vpoint* out_host, int cap, int* n_out);

/* ---- readout: dsp_dynamic.h:385-438 ---- */
/* getOccupancyMap :385-402 : voxel centres with occupancy mass > thr, ascending voxel
 * index; ALSO zeroes the future accumulators like the reference (:397-400). */
int dspmap_get_occupancy(dspmap_t* m, float threshold, float* xyz_out_host, int cap, int* n_out);
/* getOccupancyMapWithFutureStatus :405-426 : as above + copies V x T future masses, then zeroes them */
int dspmap_get_occupancy_with_future(dspmap_t* m, float threshold, float* xyz_out_host, int cap, int* n_out,
                                     float* future_status_host /* [V_local][T] */);
/* north-star name getFutureStatus(): the V x T copy + zeroing only */
int dspmap_get_future(dspmap_t* m, float* future_status_host);
/* clearOccupancyMapPrediction :431-438 */
int dspmap_clear_future(dspmap_t* m);
/* voxels_objects_number[v][0..3] (:118-120): occupancy mass + mean velocity, V_local x 4 floats */
int dspmap_get_results(dspmap_t* m, float* out_host);
/* device-resident views for callers that keep the map on the GPU (no copy) */
const float* dspmap_results_device(dspmap_t* m); /* [V_local][4] */
const float* dspmap_future_device(dspmap_t* m);  /* [V_local][T] */

/* ---- point and trajectory queries (no counterpart in the reference; a planner's question "what is predicted around these
 * points at these times?" answered on the device without the whole-grid copy above).  READ-ONLY: a query never clears the future
 * accumulators and never arms the clear that getOccupancyMap* leave behind (:397-400, :420-424); a later dspmap_get_future of the same
 * frame returns the same grid, and no later frame computes anything differently.
 *
 * A sample is {x, y, z, t} (16 bytes).  Its value:
 *  - frame: x, y, z are in the map frame (relative to the map centre, like dspmap_voxel_center and the occupancy cloud); with
 *    flags & DSPMAP_QUERY_WORLD they are world coordinates and each axis is first reduced p = fl(q - cur_pos), cur_pos = the sensor
 *    position of the last update (or dspmap_set_current_position).
 *  - which value: t < 0 reads the current mass voxels_objects_number[v][0] (dspmap_get_results column 0); t >= 0 reads the future
 *    status at horizon k(t) = the smallest k with prediction_future_time[k] >= t, clamped to T - 1: bit for bit the [v][k] entry of
 *    dspmap_get_future -- or 0 while a clear is pending (after a consuming readout or dspmap_clear_future), as the reference's zeroed
 *    cells would read.  A map with T == 0 reads the current mass for every t.
 *  - footprint: the MAXIMUM of (a) the own voxel's value if the point is inside the map (dspmap_point_voxel_index's voxel), and
 *    (b) the value of every voxel-centre lattice point (ix, iy, iz) with d2 <= fl(r * r), where the centre c is dspmap_voxel_center's
 *    fl(fl((float)i * res) + (-half + res / 2)) per axis (extended to indices outside the map), d = fl(c - p) per axis and
 *    d2 = fl(fl(fl(dx * dx) + fl(dy * dy)) + fl(dz * dz)).  A lattice point outside [0, nx) x [0, ny) x [0, nz) contributes
 *    `outside_value`, and so does a point outside the map.  A sample with a NaN coordinate or t has the value `outside_value`.
 *    r == 0: the own voxel, or `outside_value`.  0 <= r <= 8 * voxel_resolution, anything else is DSPMAP_E_ARG.
 *  - sharded handles (slab [z_lo, z_hi)): only voxels of the handle's slab contribute a mass; the outside contributions apply on
 *    every slab; a sample with no contribution on this slab reads -inf.  The elementwise max of all slabs' outputs is the unsharded
 *    map's output.
 * Arguments are checked before the device is touched: a NULL handle, n < 0, a NULL array with n > 0, a bad r, unknown flags or a
 * NaN outside_value are DSPMAP_E_ARG; without a usable device a valid call is DSPMAP_E_DEVICE.  Work is queued on the handle's
 * stream behind everything queued there before (the last frame included); the captured frame is not touched. */
#define DSPMAP_QUERY_WORLD 1
typedef struct dspmap_query {
    float x, y, z, t;
} dspmap_query;
typedef struct dspmap_risk {
    float sum;        /* fp32 sum of the trajectory's sample values, taken sequentially in sample order */
    float max;        /* their maximum */
    int first_over;   /* first sample whose value is > threshold (getOccupancyMap's comparison, :394), -1 if none */
    int n_outside;    /* samples whose point is outside the map or that have a NaN coordinate or t */
} dspmap_risk;
/* out_host[i] = value of q_host[i]; synchronous */
int dspmap_query_occupancy(dspmap_t* m, int n, const dspmap_query* q_host, float radius, int flags, float outside_value,
                           float* out_host);
/* the same on device arrays (q_dev: n x 16 B, out_dev: n floats); enqueued on the handle's stream, no synchronisation */
int dspmap_query_occupancy_device(dspmap_t* m, int n, const dspmap_query* q_dev, float radius, int flags, float outside_value,
                                  float* out_dev);
/* n_traj trajectories of n_samples samples each, trajectory-major (q[t * n_samples + j]) -> one dspmap_risk per trajectory from the
 * values above.  n_samples <= 0 with n_traj > 0, or more than INT_MAX samples in all, is DSPMAP_E_ARG; a sharded handle is
 * DSPMAP_E_STATE (a trajectory's sum needs every slab).  Synchronous */
int dspmap_trajectory_risk(dspmap_t* m, int n_traj, int n_samples, const dspmap_query* q_host, float radius, int flags,
                           float outside_value, float threshold, dspmap_risk* out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_trajectory_risk_device(dspmap_t* m, int n_traj, int n_samples, const dspmap_query* q_dev, float radius, int flags,
                                  float outside_value, float threshold, dspmap_risk* out_dev);

/* ---- truncated Euclidean distance fields of the current and the predicted occupancy (no counterpart in the reference; the clearance a
 * gradient-based planner, an MPC cost term or a corridor generator needs right after the map, computed where the map lives instead of by
 * T + 1 whole-grid copies and CPU distance transforms).
 *
 * Layers: L = T + 1.  Layer 0 is the current mass, layer 1 + k is horizon k; a map with T == 0 has one layer.  Each layer is a dense
 * [nz][ny][nx] grid in the reference's global voxel index order (:1081), whatever DSPMAP_P_TILING stores internally.
 *  - occupied: layer 0: voxels_objects_number[v][0] > threshold (getOccupancyMap's comparison, :394; dspmap_get_results column 0);
 *    layer 1 + k: future[v][k] > threshold with future bit for bit what dspmap_get_future would return -- 0 everywhere while a clear is
 *    pending (after a consuming readout or dspmap_clear_future), as the queries above read it.
 *  - value: with integer voxel indices, D2(i) = min over the occupied voxels u of (ix - ux)^2 + (iy - uy)^2 + (iz - uz)^2, +inf for a layer
 *    without an occupied voxel.  With DSPMAP_DIST_OUTSIDE_OCCUPIED also the minimum over the three axes of min(i_a + 1, n_a - i_a)^2: the
 *    lattice just outside the map counts as occupied, which pushes a planner away from the edge of the local map.
 *    d2c = min(D2, R^2) with R = max_voxels, and the value is fl(fl(sqrtf((float)d2c)) * voxel_resolution), sqrt correctly rounded.  All
 *    integers involved are <= 4096: everything up to the sqrt is exact and the field is defined bit for bit.
 *  - arguments, checked before the device is touched: a NULL handle, a NaN threshold, max_voxels outside 1 .. 64 or unknown flags are
 *    DSPMAP_E_ARG; a sharded handle (slab) is DSPMAP_E_STATE (distances cross slabs); without a usable device a valid call is
 *    DSPMAP_E_DEVICE.
 *  - snapshot: the build is enqueued on the handle's stream behind everything queued there before (the last frame included) and does not
 *    synchronise.  It writes into a buffer the handle owns (the buffer and two scratch grids of 1 and 2 bytes per cell are allocated by
 *    the first build; a handle that never builds a field allocates nothing).  READ-ONLY towards the map: no accumulator is cleared, the
 *    pending clear is neither armed nor carried out, the captured frame and its parameter ring are not touched.  The field stays valid
 *    through readouts and dspmap_clear_future (it is a snapshot of the frame it was built from) and becomes STALE with every call that
 *    computes a new frame or replaces state: dspmap_update*, dspmap_update_depth*, dspmap_mgpu_*, dspmap_stage_predict / update / birth /
 *    resample, dspmap_import_state, dspmap_clear_state, dspmap_load_checkpoint, dspmap_add_random_particles, dspmap_seed_uniform*.  On a
 *    stale or never-built field dspmap_distance_field_device returns NULL, dspmap_get_distance_field and dspmap_query_distance* return
 *    DSPMAP_E_STATE with a text.  A `layer` outside [0, L) is DSPMAP_E_ARG.
 * dspmap_query_distance*: samples, frame convention, DSPMAP_QUERY_WORLD and the NaN rule are those of dspmap_query_occupancy.
 *  - layer: t < 0 or T == 0 selects layer 0, otherwise layer 1 + k(t) with the k(t) of dspmap_query_occupancy.
 *  - a point outside the map, or a sample with a NaN, reads `outside_value` and the gradient (0, 0, 0); otherwise the distance is the
 *    field at the point's own voxel (dspmap_point_voxel_index's voxel), and the gradient per axis, with index i of n along it:
 *    lo = max(i - 1, 0), hi = min(i + 1, n - 1), g = fl(fl(F[hi] - F[lo]) / fl((float)(hi - lo) * voxel_resolution)); g = 0 if n == 1.
 *  - a NULL handle, n < 0, a NULL sample or distance array with n > 0, unknown flags or a NaN outside_value are DSPMAP_E_ARG. */
#define DSPMAP_DIST_OUTSIDE_OCCUPIED 1
int dspmap_build_distance_field(dspmap_t* m, float threshold, int max_voxels, int flags);
const float* dspmap_distance_field_device(dspmap_t* m);            /* [L][V] device memory, NULL if none / stale */
int dspmap_get_distance_field(dspmap_t* m, int layer, float* out_host);   /* V floats; synchronous */
/* dist_out_host[i], grad_out_host[3 i .. 3 i + 2] (n x 3, may be NULL) of q_host[i]; synchronous */
int dspmap_query_distance(dspmap_t* m, int n, const dspmap_query* q_host, int flags, float outside_value, float* dist_out_host,
                          float* grad_out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_query_distance_device(dspmap_t* m, int n, const dspmap_query* q_dev, int flags, float outside_value, float* dist_out_dev,
                                 float* grad_out_dev);

/* ---- nearest-obstacle fields: WHICH voxel the closest obstacle is, and the signed distance to it (no counterpart in the reference; what a
 * gradient-based avoider, a velocity-obstacle or a CBF constraint joins to the per-voxel velocities of dspmap_get_results, instead of a
 * whole-grid copy and a CPU distance transform with indices per layer).  The distance field above is zero, with a zero gradient, inside
 * obstacles and names no obstacle; this layer does both.
 *
 * Layers: those of the distance field.  L = T + 1, layer 0 the current mass, layer 1 + k horizon k; each a dense [nz][ny][nx] grid in the
 * reference's global voxel index order (:1081), whatever DSPMAP_P_TILING stores internally.
 *  - occupied set of a layer.  Without DSPMAP_NEAREST_FROM_CAST_GRID: the distance field's rule -- layer 0: voxels_objects_number[v][0] >
 *    threshold; layer 1 + k: future[v][k] > threshold, bit for bit what dspmap_get_future returns, and 0 everywhere while a clear is pending.
 *    With DSPMAP_NEAREST_FROM_CAST_GRID: the bits of the VALID cast grid as it is now -- inflated, masked with unknown space
 *    (dspmap_mask_cast_grid) or replaced by dspmap_debug_set_cast_grid; `threshold` is then not read.  The nearest obstacle is then
 *    consistent with what casts, boxes and wavefronts call blocked.
 *  - target set of a cell.  A free cell targets the occupied voxels of its layer.  An occupied cell without DSPMAP_NEAREST_SIGNED targets
 *    itself (D2 = 0).  An occupied cell with DSPMAP_NEAREST_SIGNED targets the FREE voxels inside the map; padding bits at x >= nx and the
 *    lattice outside the map belong to neither set.
 *  - near[i].  With integer voxel indices D2(i) = min over the targets u of (ix - ux)^2 + (iy - uy)^2 + (iz - uz)^2.  If D2 > R^2 with
 *    R = max_voxels, or there is no target, near = -1 (D2 == R^2 is a valid target).  Otherwise near is the global index of the minimiser;
 *    among several, the smallest global voxel index: smallest uz, then smallest uy, then smallest ux.
 *  - dist[i].  d2c = min(D2, R^2), R^2 when there is no target; the value is fl(fl(sqrtf((float)d2c)) * voxel_resolution), sqrt correctly
 *    rounded, NEGATED for an occupied cell under DSPMAP_NEAREST_SIGNED (its D2 is at least 1: there is no -0).  Without either flag dist
 *    equals the field of dspmap_build_distance_field(threshold, max_voxels, 0) bit for bit.  All integers involved are <= 4096: both
 *    grids are defined bit for bit.
 *  - arguments, checked in the order of dspmap_build_objects: a NULL handle, a NaN threshold without DSPMAP_NEAREST_FROM_CAST_GRID,
 *    max_voxels outside 1 .. 64 or unknown flags are DSPMAP_E_ARG; then a sharded handle (slab) is DSPMAP_E_STATE; then
 *    DSPMAP_NEAREST_FROM_CAST_GRID without a valid cast grid is DSPMAP_E_STATE with a text naming dspmap_build_cast_grid; without a usable
 *    device a valid call is DSPMAP_E_DEVICE.
 *  - snapshot: the life cycle of the distance field.  The build is enqueued on the handle's stream behind everything queued there before
 *    and does not synchronise (except where a first or a larger build has to allocate).  It writes two [L][V] grids the handle owns
 *    (allocated by the first build, with scratch of 1 and 4 bytes per cell and layer, twice that for a signed build; a handle that never
 *    builds one allocates nothing).  READ-ONLY towards the map in every sense listed for the distance field, and towards the cast grid
 *    and the distance field of the handle.  It stays valid through readouts and dspmap_clear_future and becomes STALE with every call
 *    that makes a distance field stale.  A snapshot built with DSPMAP_NEAREST_FROM_CAST_GRID also becomes stale with everything that
 *    replaces or changes the cast grid: dspmap_build_cast_grid, dspmap_mask_cast_grid, dspmap_debug_set_cast_grid; a snapshot built from
 *    the masses does not depend on the cast grid.  On a stale or never-built snapshot dspmap_nearest_field_device and
 *    dspmap_nearest_distance_device return NULL, dspmap_get_nearest_field and dspmap_query_nearest* return DSPMAP_E_STATE with a text
 *    naming dspmap_build_nearest_field.  dspmap_get_nearest_field: either output may be NULL, not both (DSPMAP_E_ARG); a `layer`
 *    outside [0, L) is DSPMAP_E_ARG.
 * dspmap_query_nearest*: samples, frame convention, DSPMAP_QUERY_WORLD, the NaN rule and the layer k(t) are those of dspmap_query_distance.
 *  - a point outside the map, or a sample with a NaN, gives {outside_value, -1, 0, 0, 0, 0, 0, 0}.
 *  - otherwise, with g the point's own voxel (dspmap_point_voxel_index's voxel) and p the reduced point: dist = dist[g], voxel = near[g];
 *    the offset to the centre of the nearest voxel o_a = fl(c_a(voxel) - p_a) per axis, c = dspmap_voxel_center's
 *    fl(fl((float)i * res) + (-half + res / 2)), and (0, 0, 0) when voxel == -1.
 *  - velocity: columns 1 .. 3 of dspmap_get_results at the OCCUPIED voxel of the pair, bit for bit, whatever storage order the handle
 *    uses: that voxel is `voxel` for a free own cell and g for an occupied one.  Filled only when the selected layer is 0 and that voxel
 *    exists (a free cell with voxel == -1 has none); (0, 0, 0) otherwise.
 *  - a NULL handle, n < 0, a NULL array with n > 0, unknown flags or a NaN outside_value are DSPMAP_E_ARG. */
#define DSPMAP_NEAREST_SIGNED 1
#define DSPMAP_NEAREST_FROM_CAST_GRID 2
int dspmap_build_nearest_field(dspmap_t* m, float threshold, int max_voxels, int flags);
const int* dspmap_nearest_field_device(dspmap_t* m);        /* [L][V] int32 device memory, NULL if none / stale */
const float* dspmap_nearest_distance_device(dspmap_t* m);   /* [L][V] float device memory, NULL if none / stale */
/* V ints and / or V floats of one layer (either may be NULL, not both); synchronous */
int dspmap_get_nearest_field(dspmap_t* m, int layer, int* near_out_host, float* dist_out_host);
typedef struct dspmap_nearest {
    float dist;         /* the (signed) distance of the own voxel, metres */
    int voxel;          /* global index of its nearest target, -1 if none within max_voxels */
    float ox, oy, oz;   /* centre of `voxel` minus the point */
    float vx, vy, vz;   /* velocity of the occupied voxel of the pair (layer 0 only) */
} dspmap_nearest;       /* 32 bytes */
/* out_host[i] of q_host[i]; synchronous */
int dspmap_query_nearest(dspmap_t* m, int n, const dspmap_query* q_host, int flags, float outside_value, dspmap_nearest* out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_query_nearest_device(dspmap_t* m, int n, const dspmap_query* q_dev, int flags, float outside_value, dspmap_nearest* out_dev);

/* ---- segment casts through the current and the predicted occupancy (no counterpart in the reference; a planner's edge check, a
 * line-of-sight test or a first hit along a ray, answered where the map lives instead of by sampling dspmap_trajectory_risk every half
 * voxel -- which misses voxels a segment only clips -- or by copying the whole grid out and walking it on the host).
 *
 * Cast grid (dspmap_build_cast_grid): a snapshot with the life cycle of the distance field.  L = T + 1 layers, layer 0 the current mass,
 * layer 1 + k horizon k; each layer one bit per voxel in the reference's index order (:1081), whatever DSPMAP_P_TILING stores internally:
 * W = ceil(nx / 64) 64-bit words per row, bit (x & 63) of word (x >> 6) of row (z, y) belongs to voxel (x, y, z); bits at x >= nx are 0.
 *  - raw occupancy: the distance field's rule.  Layer 0: voxels_objects_number[v][0] > threshold (:394); layer 1 + k: future[v][k] >
 *    threshold with future bit for bit what dspmap_get_future returns -- 0 everywhere while a clear is pending.
 *  - inflation by r = inflate_voxels (0 .. DSPMAP_CAST_MAX_INFLATE), the Chebyshev ball: bit i is set iff some voxel u INSIDE the map with
 *    max over the axes of |i_a - u_a| <= r is raw-occupied.  The outside of the map contributes nothing.
 *  - arguments, checked before the device is touched: a NULL handle, a NaN threshold, inflate_voxels outside 0 .. 8 or flags != 0 are
 *    DSPMAP_E_ARG; then a sharded handle (slab) is DSPMAP_E_STATE (casts cross slabs); without a usable device a valid call is
 *    DSPMAP_E_DEVICE.
 *  - snapshot: enqueued on the handle's stream behind everything queued there before, no synchronisation.  The grid and one scratch grid
 *    of the same size (L * nz * ny * W words each) are allocated by the first build; a handle that never builds one allocates nothing.
 *    READ-ONLY towards the map in every sense listed for the distance field: no accumulator is cleared, the pending clear is neither armed
 *    nor carried out, the captured frame and its parameter ring are not touched.  The grid stays valid through readouts and
 *    dspmap_clear_future and becomes STALE with exactly the calls that make a distance field stale (dspmap_build_distance_field above).  On
 *    a stale or never-built grid dspmap_cast_grid_device returns NULL, dspmap_get_cast_grid and dspmap_cast_segments* return
 *    DSPMAP_E_STATE with a text naming dspmap_build_cast_grid.  A `layer` outside [0, L) or a NULL output is DSPMAP_E_ARG.
 *
 * A cast (dspmap_cast_segments*) walks the segment a -> b, parameter s in [0, 1], through the grid cell by cell (Amanatides-Woo) and
 * reports the first cell whose bit is set.  ta, tb are the times at which a and b are reached: the cell entered at parameter s is tested
 * in the horizon of the time the segment is there.  Every named operation below is rounded to fp32 on its own.
 *  1. validity, frame: a non-finite ax .. bz or a NaN ta or tb gives {0, -1, -1, DSPMAP_CAST_INVALID}.  With DSPMAP_QUERY_WORLD both end
 *     points are reduced p = fl(q - cur_pos) per axis, as in the queries.
 *  2. voxel coordinates, per axis: u_a = fl(fl(a + half) / res), u_b = fl(fl(b + half) / res) (dspmap_point_voxel_index's expression).  If
 *     dspmap_point_voxel_index calls a outside, or trunc(u_a) >= n on some axis, the result is {0, -1, -1, DSPMAP_CAST_START_OUTSIDE}.
 *     b may lie anywhere.  The start cell is i = trunc(u_a).
 *  3. set-up, per axis: d = fl(u_b - u_a), step = sign(d).  d == 0: tMax = +inf.  Otherwise bnd = (float)(i + (step > 0 ? 1 : 0)),
 *     tMax = fl(fl(bnd - u_a) / d), tDelta = fl(1.0f / fabsf(d)).  s_in = 0 for the start cell.
 *  4. per cell: the axis m with the smallest tMax leaves first, ties to x, then y, then z (tMax_x <= tMax_y && tMax_x <= tMax_z, then
 *     tMax_y <= tMax_z).  s_out = fminf(tMax_m, 1).  Layers tested: ta < 0 or T == 0: layer 0 only.  Otherwise dt = fl(tb - ta),
 *     t_in = fl(ta + fl(s_in * dt)), t_out = fl(ta + fl(s_out * dt)), and the layers 1 + k(t_in), 1 + k(t_out) (the k(t) of
 *     dspmap_query_occupancy; a t that is negative or NaN selects layer 0) and every layer between them, in ascending order.  The first
 *     tested layer whose bit is set ends the cast with {s_in, global voxel index, that layer, DSPMAP_CAST_HIT}.  If none is set:
 *     !(tMax_m <= 1) ends it with {1, -1, -1, DSPMAP_CAST_FREE}; otherwise s_in = tMax_m, i_m += step_m, tMax_m = fl(tMax_m + tDelta_m), and
 *     if i_m has left [0, n_m) the cast ends with {s_in, index of the last cell inside the map, -1, DSPMAP_CAST_LEFT_MAP}.
 *     A cast takes at most nx + ny + nz steps: each step moves one index monotonically.
 *  - arguments: a NULL handle, n < 0, a NULL array with n > 0 or flags other than DSPMAP_QUERY_WORLD are DSPMAP_E_ARG. */
#define DSPMAP_CAST_MAX_INFLATE 8
typedef struct dspmap_segment {
    float ax, ay, az, ta, bx, by, bz, tb;
} dspmap_segment; /* 32 bytes */
typedef struct dspmap_cast_hit {
    float s;      /* parameter at which the reported cell is entered (HIT, LEFT_MAP: at which the map is left), 1 for FREE, 0 otherwise */
    int voxel;    /* global voxel index of the cell (HIT: the occupied one, LEFT_MAP: the last one inside the map), else -1 */
    int layer;    /* HIT: the layer whose bit was set, else -1 */
    int status;   /* DSPMAP_CAST_* */
} dspmap_cast_hit; /* 16 bytes */
enum { DSPMAP_CAST_FREE = 0, DSPMAP_CAST_HIT = 1, DSPMAP_CAST_LEFT_MAP = 2, DSPMAP_CAST_START_OUTSIDE = 3, DSPMAP_CAST_INVALID = 4 };
int dspmap_build_cast_grid(dspmap_t* m, float threshold, int inflate_voxels, int flags /* must be 0 */);
const unsigned long long* dspmap_cast_grid_device(dspmap_t* m);          /* [L][nz][ny][W] words, NULL if none / stale */
int dspmap_get_cast_grid(dspmap_t* m, int layer, unsigned long long* out_host);   /* nz * ny * W words; synchronous */
/* out_host[i] = the cast of seg_host[i]; synchronous */
int dspmap_cast_segments(dspmap_t* m, int n, const dspmap_segment* seg_host, int flags, dspmap_cast_hit* out_host);
/* the same on device arrays (seg_dev: n x 32 B, out_dev: n x 16 B); enqueued on the handle's stream, no synchronisation */
int dspmap_cast_segments_device(dspmap_t* m, int n, const dspmap_segment* seg_dev, int flags, dspmap_cast_hit* out_dev);

/* ---- axis-aligned free boxes in the cast grid: safe corridors (no counterpart in the reference; the step a corridor planner takes right
 * after the map -- around every piece of a candidate path the largest box of free voxels, which becomes the constraint set of its
 * optimiser -- answered where the map lives instead of by a grid copy per frame and a host loop per box).
 *
 * A seed is a dspmap_segment: the piece a -> b of a path, reached at the times ta, tb -- what dspmap_cast_segments takes, so that an edge
 * check and its corridor box come from one grid and one batch.  The box is grown in the grid of the last dspmap_build_cast_grid, pure
 * integer work on its bits:
 *  1. validity, frame: the rules of dspmap_cast_segments step 1 unchanged.  A non-finite ax .. bz or a NaN ta or tb gives
 *     {-1 x 6, DSPMAP_BOX_INVALID, 0}; with DSPMAP_QUERY_WORLD both end points are reduced p = fl(q - cur_pos) per axis.
 *  2. seed box: per axis i_a = trunc(u_a), i_b = trunc(u_b) with the u_a, u_b of cast step 2.  BOTH end points must lie inside the map: if
 *     dspmap_point_voxel_index calls a or b outside, or trunc(u) >= n on some axis for either, the result is
 *     {-1 x 6, DSPMAP_BOX_SEED_OUTSIDE, 0}.  The seed box is lo = min(i_a, i_b), hi = max(i_a, i_b) per axis.
 *  3. layers tested: the rule of cast step 4 with t_in = ta and t_out = tb.  ta < 0 or T == 0: layer 0 only.  Otherwise the layers
 *     1 + k(ta), 1 + k(tb) (the k(t) of dspmap_query_occupancy; a negative tb selects layer 0) and every layer between them.  With
 *     DSPMAP_BOX_WITH_CURRENT layer 0 is tested in addition.  A cell is BLOCKED iff its bit is set in some tested layer.
 *  4. seed test: if a cell of the seed box is blocked the result is {seed box, DSPMAP_BOX_SEED_BLOCKED, 0}.
 *  5. growth: all six faces f = 0 .. 5 (-x, +x, -y, +y, -z, +z) start active; rounds are repeated until none is.  A round visits the
 *     faces in the order f = 0 .. 5 and skips the inactive ones.  For an active face on axis a, c = lo_a - 1 or hi_a + 1, tested in this
 *     order: (i) c outside [0, n_a) stops the face with cause DSPMAP_BOX_STOP_EDGE; (ii) c farther than max_grow[a] from the SEED box's
 *     bound on that side (seed lo_a - c, or c - seed hi_a, > max_grow[a]) stops it with DSPMAP_BOX_STOP_LIMIT; (iii) a blocked cell in the
 *     slab {index c on axis a} x the current [lo, hi] on the other two axes -- extensions made earlier in the same round included --
 *     stops it with DSPMAP_BOX_STOP_OBSTACLE; otherwise the box is extended to c.  A stopped face is inactive for good and its cause is
 *     recorded in `stop`.  That is exact, not a heuristic: the slab of a stopped face only grows afterwards, so its obstacle stays in it.
 *     The result is {box, DSPMAP_BOX_OK, stop}; no cell of the box is blocked.  At most 6 * (DSPMAP_BOX_MAX_GROW + 1) face tests per seed.
 *  - inflation is whatever the grid was built with: a box grown in a grid inflated by r keeps a Chebyshev distance greater than r voxels
 *    from every raw-occupied voxel of the tested layers.
 *  - arguments, checked before the device is touched: a NULL handle, n < 0, a NULL array with n > 0, a NULL max_grow, a max_grow[a] outside
 *    0 .. DSPMAP_BOX_MAX_GROW or flags outside DSPMAP_QUERY_WORLD | DSPMAP_BOX_WITH_CURRENT are DSPMAP_E_ARG.  Then, as for
 *    dspmap_cast_segments: a sharded handle (slab) is DSPMAP_E_STATE; a stale or never-built grid is DSPMAP_E_STATE with a text naming
 *    dspmap_build_cast_grid (without a usable device there is no grid: dspmap_build_cast_grid is the call that reports DSPMAP_E_DEVICE);
 *    a device call that fails is DSPMAP_E_DEVICE.
 *  - state: READ-ONLY towards the map and the grid; what makes the grid stale is unchanged and a call does not make it so.  Enqueued on
 *    the handle's stream behind the build and the frame. */
#define DSPMAP_BOX_MAX_GROW 64
#define DSPMAP_BOX_WITH_CURRENT 2          /* flag; DSPMAP_QUERY_WORLD (1) is the other one */
typedef struct dspmap_box {
    int lo[3], hi[3];   /* inclusive voxel indices x, y, z; -1 everywhere for SEED_OUTSIDE / INVALID */
    int status;         /* DSPMAP_BOX_* */
    unsigned stop;      /* 2 bits per face f = 0..5 (-x, +x, -y, +y, -z, +z) at bits 2f, 2f+1: why growth ended there */
} dspmap_box;           /* 32 bytes */
enum { DSPMAP_BOX_OK = 0, DSPMAP_BOX_SEED_BLOCKED = 1, DSPMAP_BOX_SEED_OUTSIDE = 3, DSPMAP_BOX_INVALID = 4 };
enum { DSPMAP_BOX_STOP_OBSTACLE = 1, DSPMAP_BOX_STOP_EDGE = 2, DSPMAP_BOX_STOP_LIMIT = 3 };
/* out_host[i] = the box of seed_host[i]; synchronous */
int dspmap_grow_boxes(dspmap_t* m, int n, const dspmap_segment* seed_host, const int max_grow[3], int flags, dspmap_box* out_host);
/* the same on device arrays (seed_dev: n x 32 B, out_dev: n x 32 B; max_grow is host memory); enqueued on the handle's stream, no
 * synchronisation */
int dspmap_grow_boxes_device(dspmap_t* m, int n, const dspmap_segment* seed_dev, const int max_grow[3], int flags, dspmap_box* out_dev);

/* ---- arrival-time fields: a space-time wavefront through the cast grid (no counterpart in the reference; the global question behind the
 * local ones above -- from where the robot is, through the occupancy the map predicts, which cells can it reach, and how early?  Grown from
 * a goal the same field is the cost-to-go a search uses as its heuristic and a local planner descends -- answered where the map lives
 * instead of by a grid copy per frame and a BFS on the host).
 *
 * A build grows n_fields fields, each from its own source points, in the grid of the last dspmap_build_cast_grid (inflated as that grid
 * is).  Exact integer work on its bits:
 *  - cells, neighbours: the cells are the voxels of the map, the neighbours N6 of a cell its six face neighbours INSIDE the map.  The
 *    outside of the map does not exist; bits at x >= nx are never reached.
 *  - schedule: step n = 0, 1, ... happens at the time t_n = fl(t_start + fl((float)n * step_seconds)).  If t_start < 0 or T == 0 every
 *    step tests layer 0; otherwise step n tests layer 1 + k(t_n) with the k(t) of dspmap_query_occupancy (monotone in n, clamped at the
 *    last horizon).  With DSPMAP_REACH_WITH_CURRENT layer 0 is tested in addition.  B_n = the cells whose bit is set in a layer tested at
 *    step n.
 *  - sources: a dspmap_reach_point {x, y, z, field}; frame conventions and DSPMAP_QUERY_WORLD (p = fl(q - cur_pos) per axis) are those of
 *    the queries.  Its cell is dspmap_point_voxel_index's voxel, per axis trunc(u), u = fl(fl(p + half) / res), with the trunc(u) >= n
 *    rule of cast step 2 (such a point is outside).  A source with a non-finite coordinate, outside the map or with `field` outside
 *    [0, n_fields) is ignored.  S_f = the source cells of field f.
 *  - wavefront, per field: R_0 = S_f \ B_0, R_n = (R_{n-1} u N6(R_{n-1})) \ B_n.  Waiting in place is allowed; a reached cell that
 *    becomes blocked is REMOVED, so the set is not monotone when the layers change, and a front that is blocked everywhere at one step
 *    reaches nothing afterwards.
 *  - value of a cell, uint16: the smallest n <= max_steps with the cell in R_n, or DSPMAP_REACH_UNREACHED.  Fields are
 *    [n_fields][nz][ny][nx] in the reference's voxel index order, whatever DSPMAP_P_TILING stores.
 *  - time-invariant fields: a build is time-invariant iff layer(0) == layer(max_steps) (decided on the host; the layer is monotone in n, so
 *    no step tests another one).  In such a field every cell of value v > 0 has a neighbour of value v - 1.
 *  - paths exist ONLY for time-invariant builds: when the layers change, a cell's first arrival may have come through a cell that was
 *    itself reached earlier, removed and never reached at the step needed, so first arrivals alone do not determine a path.
 *    A start is a dspmap_reach_point.  steps_out[i] = the value of its cell; -1 if that is DSPMAP_REACH_UNREACHED, -2 if the point is
 *    outside the map, -3 if a coordinate is non-finite or `field` is outside [0, n_fields) (-3 wins over -2).
 *    cells_out[i * max_len + j] are global voxel indices: j = 0 the start's cell, cell j + 1 the FIRST neighbour of cell j in the order
 *    -x, +x, -y, +y, -z, +z whose value is one less.  The path ends at a cell of value 0 or after max_len cells; the remaining entries,
 *    and all of them when steps_out[i] < 0, are -1.  Should no neighbour qualify the path stops there and the rest is -1: no loop is
 *    unbounded.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text: a NULL handle, n_fields outside
 *    1 .. DSPMAP_REACH_MAX_FIELDS, n_src < 0, a NULL array with n_src > 0, a NaN t_start, a step_seconds that is NaN, negative or infinite,
 *    max_steps outside 1 .. DSPMAP_REACH_MAX_STEPS, flags outside DSPMAP_QUERY_WORLD | DSPMAP_REACH_WITH_CURRENT |
 *    DSPMAP_REACH_DEVICE_SETS, n_fields * V > 2^31.  Paths: n < 0, max_len outside 0 .. DSPMAP_REACH_MAX_STEPS + 1, a NULL start or
 *    steps_out with n > 0, a NULL cells_out with n > 0 and max_len > 0, flags other than DSPMAP_QUERY_WORLD, n * max_len > 2^31.
 *  - state, after the arguments and in dspmap_grow_boxes' order: a sharded handle (slab) is DSPMAP_E_STATE; a build on a stale or
 *    never-built grid is DSPMAP_E_STATE with a text naming dspmap_build_cast_grid (without a usable device there is no grid); the accessors
 *    and the paths on a stale or never-built snapshot are DSPMAP_E_STATE with a text naming dspmap_build_reach_fields; paths on a build that
 *    is not time-invariant are DSPMAP_E_STATE with a text saying so.  A device call that fails is DSPMAP_E_DEVICE.
 *  - life cycle: the snapshot goes stale with everything that makes the cast grid stale, with every dspmap_build_cast_grid and with
 *    dspmap_debug_set_cast_grid.  READ-ONLY towards the map and the grid in every sense listed for dspmap_grow_boxes.  The buffers are
 *    allocated by the first build (grown by a larger one) and freed with the device state; a handle that never builds allocates nothing.
 *    Enqueued on the handle's stream behind the grid's build and the frame. */
#define DSPMAP_REACH_MAX_FIELDS 64
#define DSPMAP_REACH_MAX_STEPS 4096
#define DSPMAP_REACH_UNREACHED 65535
#define DSPMAP_REACH_WITH_CURRENT 2        /* flag; DSPMAP_QUERY_WORLD (1) is the other public one */
#define DSPMAP_REACH_DEVICE_SETS 4         /* diagnostic flag: keep the wave sets in device memory even where they fit in LDS; same result */
typedef struct dspmap_reach_point {
    float x, y, z;
    int field;
} dspmap_reach_point;   /* 16 bytes */
/* grow n_fields fields from src_host[0 .. n_src); synchronous */
int dspmap_build_reach_fields(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_host, float t_start, float step_seconds,
                              int max_steps, int flags);
/* the same on a device array (src_dev: n_src x 16 B); enqueued on the handle's stream, no synchronisation */
int dspmap_build_reach_fields_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_dev, float t_start,
                                     float step_seconds, int max_steps, int flags);
/* device address of the [n_fields][V] uint16 values of the last build; NULL if there is none or it is stale */
const unsigned short* dspmap_reach_fields_device(dspmap_t* m);
/* out_host[0 .. V) = the values of one field of the last build; synchronous */
int dspmap_get_reach_field(dspmap_t* m, int field, unsigned short* out_host);
/* paths of n starts down a time-invariant build: steps_out[n], cells_out[n * max_len] (may be NULL when max_len == 0); synchronous */
int dspmap_reach_paths(dspmap_t* m, int n, const dspmap_reach_point* start_host, int max_len, int flags, int* steps_out_host, int* cells_out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_reach_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start_dev, int max_len, int flags, int* steps_out_dev, int* cells_out_dev);
/* diagnostic: out[0] / out[1] = the fields of the last build whose wave sets lived in LDS / in device memory */
int dspmap_debug_reach_storage(dspmap_t* m, long long out[2]);

/* ---- space-time paths: the wavefront's sets kept per step, and paths traced backwards through them (no counterpart in the reference).
 * dspmap_reach_paths refuses every build in which the tested layer changed -- the builds a dynamic map is for: a gap that opens behind a
 * passing object, a door that closes at horizon 2.  For those the first arrivals say "can I get there, and when?" but not "how?".  The
 * missing piece is exact: keep every step's set R_n where the wavefront computes it, then walk backwards through the sets.
 *
 *  - build: dspmap_build_reach_timeline* has the arguments, flags (DSPMAP_QUERY_WORLD | DSPMAP_REACH_WITH_CURRENT |
 *    DSPMAP_REACH_DEVICE_SETS), checks and check order of dspmap_build_reach_fields* and produces exactly that function's fields:
 *    dspmap_get_reach_field, dspmap_reach_fields_device, dspmap_debug_reach_storage and dspmap_reach_paths behave after it as after a plain
 *    build (dspmap_reach_paths works if the build is time-invariant and is DSPMAP_E_STATE otherwise).  In addition it keeps R_n of every
 *    step it executes, step 0 included: one row per step in the cast grid's layer layout, nz * ny * W words, bit x & 63 of word x >> 6,
 *    bits at x >= nx are 0; rows [n_fields][max_steps + 1].
 *  - one more argument check, after the existing ones and before the device is touched: n_fields * (max_steps + 1) * nz * ny * W * 8 bytes
 *    above DSPMAP_REACH_TIMELINE_MAX_BYTES is DSPMAP_E_ARG with a text that names both numbers.  The cap is a condition, not a measurement:
 *    a quarter of a percent of the card; a single field at the largest max_steps still fits on 132 x 132 x 60 (779 MB), the 64-field batch
 *    on 66 x 66 x 40 (5 280 words a step) up to max_steps 396.
 *  - early exit, last[f]: the wavefront stops a field early when its set is empty (it stays empty) or when a step changed nothing and the
 *    layer never changes again.  last[f] is the last step the field executed; for n > last[f], R_n = R_last[f] -- for both exits, because
 *    an extinguished field's last row is empty.  Rows behind last[f] are never written; dspmap_get_reach_sets serves a step in
 *    (last[f], max_steps] from row last[f], a reader of dspmap_reach_timeline_device does the same with dspmap_reach_last_steps.
 *  - dspmap_get_reach_sets copies n_steps rows from step first_step on.  DSPMAP_E_ARG: a `field` outside the build's fields,
 *    first_step < 0, n_steps < 0, first_step + n_steps > max_steps + 1, a NULL output with n_steps > 0.
 *  - timeline paths: start validity, frame, the steps_out codes (-3 invalid, -2 outside the map, -1 DSPMAP_REACH_UNREACHED) and the
 *    max_len rules are those of dspmap_reach_paths; otherwise steps_out[i] = v, the start cell's first arrival.  cells_out[i * max_len + j]
 *    is the cell occupied at step v - j; j = 0 is the start's cell.  Given cell c_j with v - j > 0, let P = R_{v-j-1} of the start's
 *    field: c_{j+1} = c_j if c_j is in P (a wait), otherwise the FIRST face neighbour inside the map, in the order -x, +x, -y, +y, -z,
 *    +z, that is in P.  One such neighbour always exists, because R_n is a subset of R_{n-1} u N6(R_{n-1}); should none qualify the path
 *    stops and the rest is -1: no loop is unbounded.  The path has v + 1 cells, one per step; it ends in a free source cell at step 0 or
 *    after max_len cells, and entries behind the end are -1.  Path flags other than DSPMAP_QUERY_WORLD are DSPMAP_E_ARG.
 *  - consequence: on a time-invariant build the sets are monotone, a chosen cell's value is exactly v - j, so the path never waits and
 *    equals dspmap_reach_paths' int for int.
 *  - state: the timeline goes stale with everything that makes the arrival fields stale, and with every plain
 *    dspmap_build_reach_fields*, which replaces the fields it belongs to.  On no timeline or a stale one the accessors and the paths are
 *    DSPMAP_E_STATE with a text naming dspmap_build_reach_timeline, and dspmap_reach_timeline_device returns NULL.  A slab handle is
 *    DSPMAP_E_STATE; without a device a valid build is DSPMAP_E_DEVICE.  READ-ONLY towards the map and the grid like the rest of the family.
 *    The buffers are allocated by the first timeline build, grown by a larger one after the stream has drained, and freed with the device
 *    state; a handle that never builds one allocates nothing.
 *  - not offered: arriving at a chosen step instead of the first one, more than one workgroup per field.  (dspmap_shorten_paths below
 *    turns a path into the few straight pieces a planner takes, waits included; it offers neither any-angle optimality nor arrival at a
 *    chosen step.) */
#define DSPMAP_REACH_TIMELINE_MAX_BYTES (1ull << 30)
/* grow the fields AND keep every step's set; synchronous */
int dspmap_build_reach_timeline(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_host, float t_start, float step_seconds,
                                int max_steps, int flags);
/* the same on a device array (src_dev: n_src x 16 B); enqueued on the handle's stream, no synchronisation */
int dspmap_build_reach_timeline_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_dev, float t_start,
                                       float step_seconds, int max_steps, int flags);
/* device address of the rows [n_fields][max_steps + 1][nz][ny][W] of the last timeline build; NULL if there is none or it is stale */
const unsigned long long* dspmap_reach_timeline_device(dspmap_t* m);
/* out_host[0 .. n_fields) = the last step each field of the last timeline build executed; synchronous */
int dspmap_reach_last_steps(dspmap_t* m, int* out_host);
/* out_host = n_steps rows of nz * ny * W words: R_first_step .. of one field; synchronous */
int dspmap_get_reach_sets(dspmap_t* m, int field, int first_step, int n_steps, unsigned long long* out_host);
/* paths of n starts backwards through the kept sets: steps_out[n], cells_out[n * max_len] (may be NULL when max_len == 0); synchronous */
int dspmap_reach_timeline_paths(dspmap_t* m, int n, const dspmap_reach_point* start_host, int max_len, int flags, int* steps_out_host,
                                int* cells_out_host);
/* the same on device arrays; enqueued on the handle's stream (behind the build: the kernel boundary orders them), no synchronisation */
int dspmap_reach_timeline_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start_dev, int max_len, int flags, int* steps_out_dev,
                                       int* cells_out_dev);
/* test hook: replace all L layers ([L][nz][ny][W] words) of the VALID cast grid.  A NULL pointer or a set bit at x >= nx is DSPMAP_E_ARG, no
 * valid grid DSPMAP_E_STATE.  The grid stays valid; arrival fields built before the call are stale.  Synchronous. */
int dspmap_debug_set_cast_grid(dspmap_t* m, const unsigned long long* words_host);

/* ---- shortened paths: a cell path cut down to line-of-sight waypoints (no counterpart in the reference).  A path from the wavefront is a
 * 6-connected staircase with one voxel per step; what a corridor generator or a trajectory optimiser takes is the few straight pieces
 * behind it.  dspmap_shorten_paths* returns, per path, a greedy farthest-visible subsequence of its cells as dspmap_segment records --
 * what dspmap_cast_segments* and dspmap_grow_boxes* take unchanged -- where the map lives, instead of a copy of the paths and the grid to the
 * host, a DDA per candidate shortcut there and an upload of the result.
 *
 *  - path i: n paths in the layout dspmap_reach_paths* and dspmap_reach_timeline_paths* produce (steps[n], cells[n * max_len]), or any
 *    caller-made polyline of cells.  v = steps[i]; v < 0: the path has no cells.  Otherwise its cells are the leading entries c_0 ..
 *    c_{m-1} of cells[i * max_len ..] that lie in [0, V): the first -1, the first out-of-range index or max_len ends the path, and
 *    m = n_cells.  Consecutive cells need not be neighbours, and equal consecutive cells (waits) are legal.
 *  - vertex: the vertex of cell c is its voxel centre, dspmap_voxel_center's expression per axis, fl(fl((float)i * res) + (-half + res / 2))
 *    (the one the query section spells out).
 *  - time: if t_start < 0 or T == 0 every vertex has the time -1.0f, so casts and boxes test layer 0.  Otherwise cell j is occupied at
 *    step e_j = max(v - j, 0) and its time is tau_j = fl(t_start + fl((float)e_j * step_seconds)), the schedule expression of
 *    dspmap_build_reach_fields: with the build's t_start and step_seconds a timeline path's cells get the times they were reached at.
 *  - cast: C(p, k) is the result dspmap_cast_segments steps 2 - 4 give for {centre(c_p), tau_p, centre(c_k), tau_k} without
 *    DSPMAP_QUERY_WORLD in the valid cast grid, inflated as that grid is -- the same instructions, not a restatement.  A wait (c_p == c_k)
 *    is a zero-length cast: it tests the layers between the two times in that one cell and nothing else.
 *  - greedy rule: start with p = 0, s = 0.  While p < m - 1: if s == max_seg, truncated = 1 and the path stops.  The candidates are
 *    k = p + 1 .. min(p + window, m - 1); q is the LARGEST candidate with C(p, k).status == DSPMAP_CAST_FREE.  If there is none, q = p + 1
 *    and n_blocked += 1: this can happen when the layer changes between two adjacent steps (or with a caller-made path through occupied
 *    cells); it is reported, not hidden.  seg_out[i * max_seg + s] = {centre(c_p), tau_p, centre(c_q), tau_q}, end_out[i * max_seg + s] = q;
 *    then p = q, s += 1.  At the end n_segments = s.
 *  - unused entries: every entry behind n_segments is written -- the segment all-zero bits, end -1 -- and so is every entry of a path with
 *    m <= 1.
 *  - consequences: the emitted vertices are a subsequence of the path, from c_0 to c_{m-1} unless truncated.  Every segment not counted
 *    in n_blocked is DSPMAP_CAST_FREE under dspmap_cast_segments bit for bit.  On a path whose consecutive cells are equal or face
 *    neighbours a segment from step e to step e' is at most |e - e'| voxels long in the sum over the axes, so the mean speed never
 *    exceeds the wavefront's one voxel per step.  On a time-invariant build the result does not depend on step_seconds.  (All of this
 *    presumes dspmap_point_voxel_index(centre(i)) == i for every voxel, which holds for the usual resolutions and is cheap to check.)
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text, in this order: a NULL handle, n < 0, max_len outside
 *    1 .. DSPMAP_REACH_MAX_STEPS + 1, window outside 1 .. DSPMAP_SHORTEN_MAX_WINDOW, max_seg < 0, flags != 0, a NaN t_start, a step_seconds
 *    that is NaN, negative or infinite, a NULL steps, cells or info array with n > 0, a NULL seg_out or end_out with n > 0 and max_seg > 0,
 *    n * max_len or n * max_seg > 2^31.
 *  - state, in dspmap_grow_boxes' order: a sharded handle (slab) is DSPMAP_E_STATE; a stale or never-built grid is DSPMAP_E_STATE with a
 *    text naming dspmap_build_cast_grid; a device call that fails is DSPMAP_E_DEVICE.
 *  - independence: the call needs the cast grid only, not a reach snapshot -- the paths may come from anywhere, also from a snapshot that
 *    has gone stale since.  READ-ONLY towards the map and the grid like dspmap_grow_boxes; it makes nothing stale and allocates nothing
 *    but the staging of the host variant.  Enqueued on the handle's stream behind the grid's build, the frame and the paths.
 *  - not offered: any-angle optimality (the vertices stay cell centres of the path, and the rule is greedy), arrival at a chosen step. */
#define DSPMAP_SHORTEN_MAX_WINDOW 64
typedef struct dspmap_path_info {
    int n_cells;      /* m: the cells the path was read with */
    int n_segments;   /* segments written, <= max_seg */
    int n_blocked;    /* of them: rounds in which no candidate was visible and the next cell was taken */
    int truncated;    /* 1: max_seg segments did not reach the last cell */
} dspmap_path_info; /* 16 bytes */
/* info_out_host[n], seg_out_host[n * max_seg], end_out_host[n * max_seg] (the last two may be NULL when max_seg == 0); synchronous */
int dspmap_shorten_paths(dspmap_t* m, int n, int max_len, const int* steps_host, const int* cells_host, float t_start, float step_seconds,
                         int window, int max_seg, int flags /* must be 0 */, dspmap_path_info* info_out_host, dspmap_segment* seg_out_host,
                         int* end_out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_shorten_paths_device(dspmap_t* m, int n, int max_len, const int* steps_dev, const int* cells_dev, float t_start, float step_seconds,
                                int window, int max_seg, int flags /* must be 0 */, dspmap_path_info* info_out_dev, dspmap_segment* seg_out_dev,
                                int* end_out_dev);

/* ---- cost-to-go fields: the wavefront weighted by clearance (no counterpart in the reference).  dspmap_build_reach_fields is a unit-cost
 * wavefront, so the paths it hands to dspmap_shorten_paths and dspmap_grow_boxes are the shortest 6-connected ones, and those hug the
 * obstacles at exactly the grid's inflation radius.  The clearance that pushes a path into the open is on the device already, per layer
 * and exact (dspmap_build_distance_field).  A build of cost fields joins the two snapshots: the step into a cell costs 1 plus a penalty from
 * the clearance band the cell lies in, the integer cost-to-go is exact, and the descent paths go out in the layout dspmap_shorten_paths*
 * takes -- instead of three copies to the host and Dijkstra there.
 *
 *  - inputs: the valid cast grid of the last dspmap_build_cast_grid (the blocked cells) and, when n_bands > 0, the valid distance field of
 *    the last dspmap_build_distance_field (the clearance).  The two are independent snapshots and may have been built with different
 *    thresholds; that is the caller's business.
 *  - layer: ONE layer l for the whole build, by the rule dspmap_build_objects has for its t: t < 0 or T == 0 selects layer 0, otherwise
 *    l = 1 + k(t) with the k(t) of dspmap_query_occupancy.  The cost fields are static in that layer.
 *  - weight of a cell c: w(c) = 0 if the bit of c is set in layer l of the cast grid (blocked); otherwise
 *    w(c) = 1 + sum over i < n_bands of penalty[i] * [F_l(c) < clearance[i]], where F_l(c) is the float the distance field stores for c in
 *    layer l and the comparison is in fp32.  Bands may nest, their order does not matter.  The distance field is truncated at
 *    R * voxel_resolution (R = its max_voxels), so a clearance above that applies to EVERY free cell -- it raises all weights alike and
 *    steers nothing.
 *  - sources: dspmap_reach_point {x, y, z, field}; the cell rule, the frame rule, DSPMAP_QUERY_WORLD and "ignored if non-finite, outside
 *    the map or with `field` outside [0, n_fields)" are those of dspmap_build_reach_fields.  A source in a blocked cell is ignored.  S_f =
 *    the free source cells of field f.
 *  - cost: the cost of a 6-connected path c_0 .. c_m inside the map with c_0 in S_f and every w(c_j) > 0 is the sum over j = 1 .. m of
 *    w(c_j), the weight of every cell ENTERED.  cost_f(c) is the minimum over such paths; a free source cell has cost 0.
 *  - value of a cell, uint16: cost_f(c) if that is <= max_cost, else DSPMAP_COST_UNREACHED.  Fields are [n_fields][nz][ny][nx] in the
 *    reference's voxel index order, whatever DSPMAP_P_TILING stores.
 *  - consequences: with n_bands == 0 the fields equal, uint16 for uint16, those of a static dspmap_build_reach_fields build of the same
 *    layer with max_steps = max_cost and without DSPMAP_REACH_WITH_CURRENT.  A cell of value v > 0 has a face neighbour of value exactly
 *    v - w(c).  For face neighbours a, b that are both reached, v(b) <= v(a) + w(b).
 *  - paths, dspmap_cost_paths*: starts and the codes of cost_out[i] are dspmap_reach_paths': the value of the start's cell, -1 if that is
 *    DSPMAP_COST_UNREACHED, -2 if the point is outside the map, -3 if a coordinate is non-finite or `field` is outside [0, n_fields)
 *    (-3 wins over -2).  cells_out[i * max_len + 0] is the start's cell; from a cell c_j of value v_j > 0 the next cell is the FIRST face
 *    neighbour inside the map, in the order -x, +x, -y, +y, -z, +z, whose value is exactly v_j - w(c_j).  The path ends at a cell of value 0
 *    or after max_len cells; the remaining entries, and all of them when cost_out[i] < 0, are -1.  Should no neighbour qualify the path
 *    stops there and the rest is -1: no loop is unbounded.  (cost_out, cells_out) is what dspmap_shorten_paths* takes as (steps, cells): use
 *    t_start = t, step_seconds = 0 for a predicted layer and t_start < 0 for layer 0.
 *  - known answer: a 10 x 3 x 1 map with nothing blocked, F = 0.05 in row y = 0 and F = 1.0 in the other rows, one band {clearance 0.1,
 *    penalty 4}, the source at cell (0, 0, 0), max_cost 100.  The values are
 *        y = 0:   0  5  8  9 10 11 12 13 14 15
 *        y = 1:   1  2  3  4  5  6  7  8  9 10
 *        y = 2:   2  3  4  5  6  7  8  9 10 11
 *    and the path from (9, 0, 0) has 12 cells: (9,0), (9,1), (8,1), ..., (0,1), (0,0).  The unweighted field reads 9 at (9, 0, 0), and its
 *    path stays in row 0.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text, in this order: a NULL handle, n_fields outside
 *    1 .. DSPMAP_COST_MAX_FIELDS, n_src < 0, a NULL array with n_src > 0, a NaN t, a NULL bands, n_bands outside 0 .. DSPMAP_COST_MAX_BANDS,
 *    a clearance[i] with i < n_bands that is NaN, infinite or <= 0, a penalty[i] with i < n_bands outside 0 .. DSPMAP_COST_MAX_WEIGHT - 1,
 *    1 + sum of penalty > DSPMAP_COST_MAX_WEIGHT, max_cost outside 1 .. DSPMAP_COST_MAX_COST, flags other than DSPMAP_QUERY_WORLD,
 *    n_fields * V > 2^31.  Paths: the argument checks of dspmap_reach_paths, max_len in 0 .. DSPMAP_REACH_MAX_STEPS + 1.
 *    DSPMAP_COST_MAX_COST is a condition, not a measurement: DSPMAP_REACH_MAX_STEPS hops at a mean weight of 4; the level loop is bounded
 *    by it.
 *  - state, after the arguments and in this order: a sharded handle (slab) is DSPMAP_E_STATE; a stale or never-built cast grid is
 *    DSPMAP_E_STATE with a text naming dspmap_build_cast_grid; with n_bands > 0 a stale or never-built distance field is DSPMAP_E_STATE
 *    with a text naming dspmap_build_distance_field (without a usable device there is neither).  The accessors and the paths on a stale or
 *    never-built snapshot are DSPMAP_E_STATE with a text naming dspmap_build_cost_fields, and the two *_device accessors return NULL.  A
 *    device call that fails is DSPMAP_E_DEVICE.
 *  - life cycle: the snapshot goes stale with everything that makes the cast grid stale, with every rebuild or in-place change of the grid
 *    (dspmap_build_cast_grid, dspmap_mask_cast_grid, dspmap_debug_set_cast_grid), with every dspmap_build_distance_field and
 *    dspmap_debug_set_distance_field -- also when the last build had n_bands == 0, so that there is one rule -- and with every new cost
 *    build.  A reach build does not touch it, and a cost build does not touch the reach snapshot.  READ-ONLY towards the map, the grid and
 *    the distance field in every sense listed for dspmap_grow_boxes.  The buffers are allocated by the first build (grown by a larger
 *    one) and freed with the device state; a handle that never builds one allocates nothing.  Enqueued on the handle's stream behind the
 *    builds of the grid and the distance field and the frame.
 *  - not offered: weights above DSPMAP_COST_MAX_WEIGHT, costs that change with time (a schedule as dspmap_build_reach_fields has), more
 *    than one workgroup per field, 26-connected or any-angle costs. */
#define DSPMAP_COST_MAX_BANDS 4
#define DSPMAP_COST_MAX_WEIGHT 8
#define DSPMAP_COST_MAX_FIELDS 64
#define DSPMAP_COST_MAX_COST 16384
#define DSPMAP_COST_UNREACHED 65535
typedef struct dspmap_cost_bands {
    int n_bands;
    float clearance[4];   /* metres, the unit of the distance field */
    int penalty[4];
} dspmap_cost_bands;   /* 36 bytes */
/* grow n_fields fields from src_host[0 .. n_src) in the layer t selects; synchronous */
int dspmap_build_cost_fields(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_host, float t, const dspmap_cost_bands* bands,
                             int max_cost, int flags);
/* the same on a device array (src_dev: n_src x 16 B; bands stays host memory and goes by value into the launch); enqueued on the handle's
 * stream, no synchronisation */
int dspmap_build_cost_fields_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src_dev, float t, const dspmap_cost_bands* bands,
                                    int max_cost, int flags);
/* device address of the [n_fields][V] uint16 values of the last build; NULL if there is none or it is stale */
const unsigned short* dspmap_cost_fields_device(dspmap_t* m);
/* out_host[0 .. V) = the values of one field of the last build; synchronous */
int dspmap_get_cost_field(dspmap_t* m, int field, unsigned short* out_host);
/* device address of the [V] uint8 weights of the last build (0 blocked, else w); NULL if there is none or it is stale */
const unsigned char* dspmap_cost_weights_device(dspmap_t* m);
/* out_host[0 .. V) = the weights of the last build; synchronous */
int dspmap_get_cost_weights(dspmap_t* m, unsigned char* out_host);
/* paths of n starts down the last build: cost_out[n], cells_out[n * max_len] (may be NULL when max_len == 0); synchronous */
int dspmap_cost_paths(dspmap_t* m, int n, const dspmap_reach_point* start_host, int max_len, int flags, int* cost_out_host, int* cells_out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_cost_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start_dev, int max_len, int flags, int* cost_out_dev, int* cells_out_dev);
/* test hook, the twin of dspmap_debug_set_cast_grid: replace all [L][V] floats of the VALID distance field.  A NULL pointer or a value that
 * is NaN, negative or infinite is DSPMAP_E_ARG, no valid field DSPMAP_E_STATE.  The field stays valid; cost fields built before the call
 * are stale.  Synchronous. */
int dspmap_debug_set_distance_field(dspmap_t* m, const float* layers_host);

/* ---- occupancy forecast at caller-chosen times from the live particle set (no counterpart in the reference, whose horizons are the
 * PREDICTION_TIMES it was compiled with; everything above snaps a time t to the next configured horizon k(t), and the future status is a
 * by-product of the resampling loop: taken from the weights before resampling, without the particles born in that frame (:944), kept in
 * consume-and-clear accumulators (:397-400, :420-424).  A planner with knots of its own -- an MPC at 20 Hz, a spline's collocation
 * times -- rolls the particles out to exactly its times instead, where they live).
 *
 * A snapshot with the life cycle of the distance field (dspmap_build_forecast), plus a point query on it.
 *  - layers: layer j is the occupancy mass at times[j] seconds after the last frame.  Each layer is a dense [nz][ny][nx] grid in the
 *    reference's voxel index order (:1081), whatever DSPMAP_P_TILING stores.  `times` is strictly ascending, every entry finite and >= 0.
 *  - who contributes: every live particle of the handle -- every set bit of the live mask (what dspmap_export_state exports), which after
 *    a frame means flags 0.6 and 1.  No weight cull and no newborn exclusion: the snapshot is of the state as it is.  A particle's
 *    quantum is q = __float2ull_rn(w * 2^24) (round to nearest even; NaN or a negative weight gives 0).
 *  - where a particle lands; every operation is rounded to fp32 on its own.  A static particle (vx == 0 && vy == 0) adds q to the voxel
 *    it is stored in, in every layer.  A moving particle, for layer j:
 *      1. fx = fl(px + fl(vx * t_j)), fy likewise;
 *      2. it contributes nothing if fabsf(fx) >= half_x or fabsf(fy) >= half_y, or if fx or fy is NaN (an import can leave a
 *         non-finite position or velocity; a particle with a NaN velocity counts as moving);
 *      3. otherwise xi = (int)fl(fl(fx + half_x) / res), yi likewise (the IEEE quotient, dspmap_point_voxel_index's expression);
 *      4. it contributes nothing if xi >= nx or yi >= ny (the one float just below half whose quotient rounds up to n, on the maps
 *         that have one);
 *      5. otherwise it adds q to voxel (xi, yi, z of the voxel it is stored in): the library's motion model has no vertical velocity
 *         (vz == 0, :661-663).  A pending vz array left by dspmap_import_state with vz != 0 is ignored.
 *  - value: (float)((double)Q * 2^-24), Q the 64-bit integer sum of the cell's quanta.  Integer sums do not depend on order: a layer is
 *    defined bit for bit -- on every run, on both storage orders, with DSPMAP_P_STATIC_TILE_SKIP 0 or 1.  The layer at t = 0 approximates
 *    dspmap_get_results column 0 but is not the same bits: that column is an fp32 sum in slot order.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text: a NULL handle, n_times outside
 *    1 .. DSPMAP_FORECAST_MAX_TIMES, a NULL `times`, a time that is NaN, infinite or negative or not greater than its predecessor,
 *    flags != 0, n_times * V >= 2^31.  Then a sharded handle (slab) is DSPMAP_E_STATE (particles cross slabs); without a usable device a
 *    valid call is DSPMAP_E_DEVICE.
 *  - snapshot: the build is enqueued on the handle's stream behind everything queued there before and does not synchronise.  READ-ONLY
 *    towards the map in every sense listed for the distance field: the future accumulators, their static part, their dirty flags and the
 *    pending clear are untouched, the captured frame and its parameter ring are untouched, no per-tile flag is written.  The buffers
 *    (the layers and n_times + 1 accumulator grids of 8 bytes per stored voxel) are allocated by the first build, grown by a larger one
 *    and freed with the device state; a handle that never builds allocates nothing.  The snapshot stays valid through readouts and
 *    dspmap_clear_future and becomes STALE with exactly the calls that make a distance field stale (dspmap_build_distance_field above).
 *    On a stale or never-built snapshot dspmap_forecast_device returns NULL, dspmap_forecast_times returns DSPMAP_E_STATE,
 *    dspmap_get_forecast and dspmap_query_forecast* return DSPMAP_E_STATE with a text naming dspmap_build_forecast.  A `layer` outside
 *    [0, n_times) or a NULL output is DSPMAP_E_ARG.
 * dspmap_query_forecast*: samples, frame convention, DSPMAP_QUERY_WORLD and the argument checks are those of dspmap_query_occupancy.
 *  - footprint: the own voxel only (dspmap_point_voxel_index's voxel); there is no radius.  A sample with a NaN coordinate or t, or a
 *    point outside the map, reads `outside_value`.
 *  - layer: j = the smallest index with times[j] >= t.  If there is none the value is layer n_times - 1; if j == 0 (this covers t < 0)
 *    the value is layer 0; otherwise, without DSPMAP_FORECAST_LERP, the value is layer j; with the flag, a = layer j - 1 and b = layer j
 *    at the voxel, u = fl(fl(t - times[j-1]) / fl(times[j] - times[j-1])) and the value is fl(a + fl(u * fl(b - a))).
 *  - flags outside DSPMAP_QUERY_WORLD | DSPMAP_FORECAST_LERP are DSPMAP_E_ARG. */
#define DSPMAP_FORECAST_MAX_TIMES 64
#define DSPMAP_FORECAST_LERP 2            /* query flag; DSPMAP_QUERY_WORLD (1) is the other one */
int dspmap_build_forecast(dspmap_t* m, int n_times, const float* times_host, int flags /* must be 0 */);
const float* dspmap_forecast_device(dspmap_t* m);                 /* [n_times][V] floats, NULL if none / stale */
int dspmap_forecast_times(dspmap_t* m, float* times_out_host, int cap);   /* returns n_times of the valid snapshot, copies min(cap, n) */
int dspmap_get_forecast(dspmap_t* m, int layer, float* out_host); /* V floats; synchronous */
/* out_host[i] = value of q_host[i]; synchronous */
int dspmap_query_forecast(dspmap_t* m, int n, const dspmap_query* q_host, int flags, float outside_value, float* out_host);
/* the same on device arrays; enqueued on the handle's stream, no synchronisation */
int dspmap_query_forecast_device(dspmap_t* m, int n, const dspmap_query* q_dev, int flags, float outside_value, float* out_dev);

/* ---- known-space layer: which voxels the sensor has seen, and when (no counterpart in the reference, which decides per frame what it can
 * see -- the rotated pyramid planes :1329-1367, the per-pyramid farthest return point_cloud_max_length, the occlusion rule of mapUpdate
 * :761 -- and keeps none of it).  The map reports a mass of 0 both for a voxel the filter has looked through and emptied and for one it
 * has never seen: behind a wall, outside the field of view, in the part of the map the vehicle has only just moved into.  This layer
 * keeps "the last frame in which the weight update reached this cell" per cell, anchored in the WORLD so that it survives ego motion.
 * It is an extension beside the frame: the frame path, its launch chain and the captured graph do not know about it.
 *
 *  - window.  Per axis a, on the host in double from the floats cur = current position (the sensor position of the last accepted
 *    update, or dspmap_set_current_position) and res = voxel_resolution, n = the map's voxels on that axis:
 *        g = cur / res - n / 2          k0 = floor(g + 0.5)  (64-bit)          o = (float)((k0 + 0.5) * res - cur)
 *    Map voxel i of that axis corresponds one-to-one to the world lattice cell k0 + i (pitch res, aligned at multiples of res); the
 *    voxel's centre always lies inside that cell.  A cell lives in slot (k0 + i) mod n (positive modulo) of a store of one 32-bit stamp
 *    per cell.  When k0 differs from the k0 the layer was last synchronised at, every lattice cell that ENTERS the window is reset to 0
 *    ("never") before anything reads or writes the layer; a shift of n or more cells on an axis resets everything.  Every entry point
 *    below synchronises first, not only dspmap_known_integrate.  A current position that is not finite is DSPMAP_E_STATE.
 *  - what a frame sees.  For cell (ix, iy, iz): p_a = fl(fl((float)i_a * res) + o_a), the cell's centre relative to the sensor.  The
 *    cell is seen when (1) it lies in a pyramid b of the frame's rotated planes (ifInPyramidsArea + findPointPyramid*Index on p,
 *    :1329-1367), (2) with dist = sqrtf(fl(fl(px * px + py * py) + pz * pz)) it is not occluded by :761, i.e. NOT (maxlen[b] > 0 and
 *    dist > fl(maxlen[b] + DSPMAP_P_OCCLUSION_MARGIN)), and (3) dist <= max_range, the caller's sensor range.  max_range = +inf gives
 *    the reference's own rule: a pyramid without a return counts as seen through, as mapUpdate treats its particles.  A cell is judged
 *    at its centre, as the reference judges a particle at its position.
 *  - stamps and ages.  A seen cell gets stamp = DSPMAP_P_UPDATE_COUNTER (>= 1); other cells keep theirs; integrating the same frame
 *    twice changes nothing.  age = update counter now - stamp, or -1 for a cell never seen.  Frames without an integration age the
 *    layer; a rejected update() changes neither the counter nor the view.
 *  - dspmap_known_integrate: enqueued on the handle's stream behind the last frame, no synchronisation.  max_range NaN or <= 0 and
 *    flags != 0 are DSPMAP_E_ARG; a sharded handle (slab) and a handle without an accepted frame are DSPMAP_E_STATE.  The store (4
 *    bytes per voxel) is allocated by the first call and freed with the device state; a handle that never calls it allocates nothing.
 *    The layer is no snapshot: it stays through frames.  dspmap_known_reset, dspmap_clear_state and dspmap_load_checkpoint forget
 *    everything (the layer is not part of a checkpoint).
 *  - dspmap_get_known: V ages in the reference's voxel order (:1081); synchronous.  Before the first integration every age is -1.
 *  - dspmap_query_known*: the age of the cell behind the voxel that holds the sample (dspmap_point_voxel_index's expression); samples,
 *    frame convention and DSPMAP_QUERY_WORLD as in dspmap_query_occupancy; t is ignored.  -1 outside the map or for a NaN coordinate.
 *    The _device variant only enqueues.
 *  - dspmap_mask_cast_grid: ORs into EVERY layer of the valid cast grid the bit of each voxel whose age is -1 or > max_age, so that
 *    casts, boxes and arrival fields treat unknown space as blocked.  Bits at x >= nx stay 0; unknown space is not inflated; arrival
 *    fields built before the call are stale.  Enqueued, no synchronisation.  max_age < 0 and flags != 0 are DSPMAP_E_ARG; a stale or
 *    never-built grid is DSPMAP_E_STATE with a text naming dspmap_build_cast_grid, a layer without an integration since its last reset
 *    DSPMAP_E_STATE with a text naming dspmap_known_integrate.
 *  - dspmap_known_stats: out[0] = cells with 0 <= age <= max_age, out[1] = cells stamped by the current frame; synchronous.
 *  - dspmap_get_view: host copies of the last frame's rotated plane normals ([(half_fov_h * 2 / angle_resolution) + 1][3] and the
 *    vertical counterpart) and of the per-pyramid farthest return ([dspmap_pyramid_num], -1 = no return); any pointer may be NULL;
 *    synchronous.
 *  Arguments are checked before the device is touched; a valid call without a usable device is DSPMAP_E_DEVICE. */
int dspmap_known_integrate(dspmap_t* m, float max_range, int flags /* must be 0 */);
int dspmap_known_reset(dspmap_t* m);
int dspmap_get_known(dspmap_t* m, int* age_out_host);             /* V ints; synchronous */
int dspmap_query_known(dspmap_t* m, int n, const dspmap_query* q_host, int flags, int* age_out_host);
int dspmap_query_known_device(dspmap_t* m, int n, const dspmap_query* q_dev, int flags, int* age_out_dev);
int dspmap_mask_cast_grid(dspmap_t* m, int max_age, int flags /* must be 0 */);
int dspmap_known_stats(dspmap_t* m, int max_age, long long out[2]);
int dspmap_get_view(dspmap_t* m, float* planes_h_host, float* planes_v_host, float* maxlen_host);

/* ---- scores of candidate viewpoints: the unknown space a frame taken from a pose would see (no counterpart in the reference).  An
 * exploration or active-perception planner asks, for some hundred candidate poses per replan: "if the sensor stood here, looking this
 * way, how many cells that are unknown now would the next frame stamp?"  Every piece of the answer is defined above: the frame's rotated
 * pyramid planes, the pyramid of a point, the occlusion rule of the known-space layer, and the segment cast.  An extension beside the
 * frame, like the sections above: the frame path, its launch chain and the captured graph do not know about it.
 *
 *  A view is {x, y, z, qw, qx, qy, qz, max_range, t}: position and DSPMAP_QUERY_WORLD as in dspmap_query_occupancy (with the flag
 *  p = fl(q - current position) per axis); the quaternion is used as given (the rotation divides by its squared norm, as the frame's
 *  does); max_range > 0, +inf allowed; t selects ONE layer of the cast grid -- layer 0 for t < 0 or a map without horizons, else layer
 *  1 + k(t) with the k(t) of dspmap_query_occupancy.  Sight is instantaneous: nothing is space-time along a ray.
 *
 *  The score is computed in the grid of the last dspmap_build_cast_grid EXACTLY AS IT IS: an inflated grid gives thicker obstacles; a
 *  grid masked with dspmap_mask_cast_grid stops the rays at unknown space, which gives the CONSERVATIVE gain (only what is certainly
 *  visible); an unmasked grid lets them pass through unknown space as through free space, the OPTIMISTIC gain.  The ages are those of
 *  the known-space layer, synchronised to the current position first like every known-space entry point.  Per view:
 *  1. validity.  A non-finite x, y, z or quaternion component, a squared norm fl(fl(fl(qx qx + qy qy) + qz qz) + qw qw) of zero, a NaN
 *     t, or a max_range that is NaN or <= 0 gives {0, 0, 0, DSPMAP_VIEW_INVALID}.  Otherwise, if dspmap_point_voxel_index calls p
 *     outside, or trunc(u_a) >= n on some axis (cast step 2), {0, 0, 0, DSPMAP_VIEW_OUTSIDE}.  Otherwise, if the bit of the view's own
 *     cell is set in the selected layer, {0, 0, 0, DSPMAP_VIEW_BLOCKED}.
 *  2. planes.  planes_h, planes_v = the handle's unrotated normals rotated by the quaternion: the frame's own expression on the frame's
 *     own tables.  A frame taken with that attitude has these planes bit for bit (dspmap_get_view).
 *  3. one ray per pyramid b = h * np_v + v.  Its unrotated direction d0 is the pyramid's centre,
 *         (1, tan alpha_h, tan beta_v) / |.|      alpha_h = (h - np_h / 2 + 0.5) step      beta_v = -(v - np_v / 2 + 0.5) step
 *     with step = angle_resolution * pi / 180, computed once on the host in double and rounded to fp32; d = d0 rotated like a plane.
 *     The ray is the cast (steps 2 - 4 of dspmap_cast_segments) of the segment a = p, b_a = fl(p_a + fl(d_a * l)), ta = tb =
 *     min(t, FLT_MAX) -- which selects the layer of step 1 in every cell -- with l = fminf(max_range, fl(res * (float)(nx + ny + nz))).
 *     A ray whose end point is not finite is no cast.  A HIT gives pyramid b the synthetic farthest return ml[b] = the distance from
 *     p to the CENTRE c of the hit voxel (dspmap_voxel_center): r_a = fl(c_a - p_a), sqrtf(fl(fl(rx rx + ry ry) + rz rz)).  Anything
 *     else gives ml[b] = -1: no return, seen through, as the known-space layer treats a pyramid without one.  n_returns = the hits.
 *     One ray per pyramid is the frame's own resolution -- it keeps one farthest return per pyramid --, so an obstacle narrower than a
 *     pyramid, far from the sensor, can be looked past.
 *  4. every voxel of the map, with c its centre and r_a = fl(c_a - p_a): b = the pyramid of r in the planes of step 2 (outside the wedge:
 *     not seen); dist as above; occluded iff ml[b] > 0 and dist > fl(ml[b] + DSPMAP_P_OCCLUSION_MARGIN); seen iff in the wedge, not
 *     occluded and dist <= max_range.  n_seen = the seen voxels; n_unknown = those of them whose age is -1 or > max_age
 *     (dspmap_mask_cast_grid's notion of unknown; ages voxel by voxel as dspmap_get_known orders them); status = DSPMAP_VIEW_OK.
 *  Everything is an integer count of exactly defined predicates: the scores are defined bit for bit and do not depend on the launch.
 *
 *  - dspmap_score_views: host arrays, synchronous.  dspmap_score_views_device: device arrays, enqueued on the handle's stream behind the
 *    build and the frame, no synchronisation.
 *  - dspmap_view_rays: what the device makes of an attitude -- planes_h [np_h + 1][3], planes_v [np_v + 1][3] and the ray directions
 *    [dspmap_pyramid_num][3]; any pointer may be NULL; synchronous; needs no grid.
 *  - dspmap_debug_view_cells (test hook): the seen set of ONE view as a bit grid [nz][ny][W] in the cast grid's word layout (bit = seen;
 *    all zero for a view that is not OK) and its ml [dspmap_pyramid_num] (may be NULL; all -1 for such a view); synchronous.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text: a NULL handle, n < 0, a NULL array with n > 0,
 *    max_age < 0, flags other than DSPMAP_QUERY_WORLD, a NULL quaternion or view.  Then, in dspmap_grow_boxes' order: a sharded handle
 *    (slab) is DSPMAP_E_STATE; a stale or never-built grid is DSPMAP_E_STATE with a text naming dspmap_build_cast_grid; a layer without
 *    an integration since its last reset is DSPMAP_E_STATE with a text naming dspmap_known_integrate (dspmap_mask_cast_grid's rule); a
 *    valid call without a usable device is DSPMAP_E_DEVICE (dspmap_view_rays; for the others there is no grid without one).  n == 0
 *    returns DSPMAP_OK and queues nothing.
 *  - read-only in every sense listed for dspmap_grow_boxes, and towards the known-space layer: nothing goes stale, the captured frame
 *    and its parameter ring are untouched.  The direction table (12 bytes per pyramid) is allocated by the first call and freed with
 *    the device state; a handle that never calls allocates nothing. */
typedef struct dspmap_view {
    float x, y, z;
    float qw, qx, qy, qz;
    float max_range;
    float t;
} dspmap_view;
typedef struct dspmap_view_score {
    int n_seen, n_unknown, n_returns;
    int status;   /* DSPMAP_VIEW_* */
} dspmap_view_score;
enum { DSPMAP_VIEW_OK = 0, DSPMAP_VIEW_BLOCKED = 1, DSPMAP_VIEW_OUTSIDE = 3, DSPMAP_VIEW_INVALID = 4 };
int dspmap_score_views(dspmap_t* m, int n, const dspmap_view* views_host, int max_age, int flags, dspmap_view_score* out_host);
int dspmap_score_views_device(dspmap_t* m, int n, const dspmap_view* views_dev, int max_age, int flags, dspmap_view_score* out_dev);
int dspmap_view_rays(dspmap_t* m, const float quat_wxyz[4], float* planes_h_host, float* planes_v_host, float* dirs_host);
int dspmap_debug_view_cells(dspmap_t* m, const dspmap_view* view_host, int flags, unsigned long long* words_out_host, float* ml_out_host);

/* ---- joint gain of views: what a SET of views sees together, and the greedy choice of k views (no counterpart in the reference).  The
 * scores above count every view as if it stood alone; a planner takes a path of poses, or the best few of some hundred candidates, and
 * views that look into the same pocket of unknown space must not be counted twice.  An extension beside the frame, like the sections
 * above: the frame path, its launch chain and the captured graph do not know about it.
 *
 *  Everything is an integer count of the predicates of dspmap_score_views.  For a view i with status DSPMAP_VIEW_OK, S_i is the set of
 *  voxels dspmap_score_views counts in n_seen (step 4; the grid dspmap_debug_view_cells returns, bit for bit) and U_i = S_i n UNK, with
 *  UNK the voxels whose age is -1 or > max_age (ages synchronised to the current position first, like every known-space entry point).  A
 *  view that is not OK has S_i = U_i = {}.  Views of one call may select different layers through t: each view's own set is defined by
 *  its own layer, and sets are united voxel by voxel.
 *
 *  - dspmap_score_view_sets: views [n_sets][set_size], dspmap_trajectory_risk's layout; a caller pads a short set with views whose
 *    max_range is 0, which are DSPMAP_VIEW_INVALID and add nothing.  Per set: n_seen = |U S_i|, n_unknown = |U U_i| (the unions over the
 *    set's members), n_ok = its OK views, reserved = 0.  scores_out (may be NULL) receives per view exactly what dspmap_score_views gives.
 *  - dspmap_select_views: views [0, n_fixed) are already committed (the rest of the plan being flown): C_0 = the union of their U_i.
 *    The candidates are [n_fixed, n).  Round r = 0 .. k - 1 computes g_i = |U_i \ C_r| for every candidate; the pick i* is the
 *    candidate with the largest g_i, among equals the one with the smallest index.  If g_i* >= min_gain, picks[r] = {i*, g_i*,
 *    |C_r u U_i*|, 0} and C_(r+1) = C_r u U_i*; otherwise this round and every later one give {-1, 0, |C_r|, 0}.  min_gain >= 1: a picked
 *    view's gain is 0 afterwards, so no view is picked twice.  n == n_fixed with k > 0 gives k empty picks.  scores_out (may be NULL)
 *    receives the n views' dspmap_score_views scores.
 *  - the _device variants take device arrays and enqueue on the handle's stream behind the build and the frame; all k rounds are
 *    enqueued, and nothing is read back between them.  They do not synchronise -- EXCEPT a call that has to allocate or grow the
 *    scratch (the handle's first call, and one with more views than the scratch holds): it waits for the stream once, because an
 *    earlier call may still use the buffers it frees.  The scratch grows to half as much again as the call needs, so batches that
 *    creep up do not wait every time.  The others take host arrays and are synchronous.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text, in this order: a NULL handle; n_sets < 0 or n < 0; a NULL
 *    view, set-score or pick array with a positive count; set_size < 1 with n_sets > 0; n_sets * set_size beyond INT_MAX; n_fixed
 *    outside [0, n]; k outside [0, DSPMAP_VIEW_MAX_PICKS]; min_gain < 1; max_age < 0; flags other than DSPMAP_QUERY_WORLD; masks beyond
 *    DSPMAP_VIEW_MASK_MAX_BYTES (below).  Then the state checks of dspmap_score_views in its order: a sharded handle, a stale or
 *    never-built grid, a layer without an integration since its last reset (all DSPMAP_E_STATE, the same texts); there is no grid
 *    without a usable device.  n_sets == 0, or n == 0 with k == 0, returns DSPMAP_OK and queues nothing.
 *  - scratch: one mask of nz * ny * W 64-bit words per view in the cast grid's word layout, and a few grids of that size; allocated by
 *    the first call, grown on demand, freed with the device state; a handle that never calls allocates nothing.  A call whose masks,
 *    views * nz * ny * W * 8 bytes, exceed DSPMAP_VIEW_MASK_MAX_BYTES is DSPMAP_E_ARG with a text that names both numbers.  The cap is a
 *    condition, not a measurement; a 132 x 132 x 60 map holds about 5 600 views under it, a 66 x 66 x 40 map about 25 000.  Masks
 *    restricted to the box of the view's max_range would lift the cap; they are not built.
 *  - read-only in every sense dspmap_score_views is: nothing goes stale, the captured frame and its parameter ring are untouched.
 *    DSPMAP_P_VIEW_CHUNKS forces the workgroups per set and per candidate too (as given, 1 .. 64, also where that is more than the
 *    layer has words for); no result depends on it. */
typedef struct dspmap_view_set_score { int n_seen, n_unknown, n_ok, reserved; } dspmap_view_set_score;
typedef struct dspmap_view_pick { int view, gain, covered, reserved; } dspmap_view_pick;
#define DSPMAP_VIEW_MAX_PICKS 64
#define DSPMAP_VIEW_MASK_MAX_BYTES (1ull << 30)
int dspmap_score_view_sets(dspmap_t* m, int n_sets, int set_size, const dspmap_view* views_host /* [n_sets][set_size] */, int max_age, int flags,
                           dspmap_view_set_score* out_host /* [n_sets] */, dspmap_view_score* scores_out_host /* [n_sets * set_size], may be NULL */);
int dspmap_score_view_sets_device(dspmap_t* m, int n_sets, int set_size, const dspmap_view* views_dev, int max_age, int flags,
                                  dspmap_view_set_score* out_dev, dspmap_view_score* scores_out_dev);
int dspmap_select_views(dspmap_t* m, int n, const dspmap_view* views_host, int n_fixed, int max_age, int flags, int k, int min_gain,
                        dspmap_view_pick* picks_out_host /* [k] */, dspmap_view_score* scores_out_host /* [n], may be NULL */);
int dspmap_select_views_device(dspmap_t* m, int n, const dspmap_view* views_dev, int n_fixed, int max_age, int flags, int k, int min_gain,
                               dspmap_view_pick* picks_out_dev, dspmap_view_score* scores_out_dev);

/* ---- frontier cells and frontier blocks: the known-free cells that touch unknown space (no counterpart in the reference).  Every
 * exploration planner starts from the frontier; block centroids are what it turns into dspmap_view candidates, so that the loop
 * update -> known_integrate -> build_cast_grid -> build_frontiers -> score_views never leaves the device.  An extension beside the
 * frame, like the sections above: the frame path, its launch chain and the captured graph do not know about it.
 *
 *  Inputs: the grid of the last dspmap_build_cast_grid EXACTLY AS IT IS (inflated, masked or replaced through
 *  dspmap_debug_set_cast_grid) and the known-space layer, synchronised to the current position first like every known-space entry
 *  point.  t selects ONE layer as for a view: layer 0 for t < 0 or a map without horizons, else layer 1 + k(t) with the k(t) of
 *  dspmap_query_occupancy.  Per voxel c, with the ages voxel by voxel as dspmap_get_known orders them:
 *     known(c)    <=>  0 <= age <= max_age
 *     unknown(c)  <=>  not known(c)                      (dspmap_mask_cast_grid's notion of unknown)
 *     free(c)     <=>  known(c) and the bit of c is clear in the selected layer
 *     u(c)         =   the number of c's six face neighbours INSIDE THE MAP that are unknown.  The outside of the map does not exist, as
 *                      for arrival fields, so 0 <= u <= 6.  Unknown is decided by age alone: the neighbour's bit is not consulted (a
 *                      masked grid has it set).
 *     frontier(c) <=>  free(c) and u(c) >= min_unknown,  min_unknown in 1 .. 6
 *  Blocks: voxel (x, y, z) belongs to block (x / block, y / block, z / block) in map indices, block in 1 ..
 *  DSPMAP_FRONTIER_MAX_BLOCK; with nb_a = ceil(n_a / block) the block index is (Z * nb_y + Y) * nb_x + X.  A block's record is {block
 *  index, count = its frontier cells, sum_x, sum_y, sum_z = the sums of their voxel indices per axis, unknown_faces = the sum of their
 *  u}: six ints.  count <= 32^3 = 2^15 and an index is < 1024 = 2^10 (dspmap_create's limits), u <= 6: every sum stays below 2^25.  The
 *  host derives a centroid as sum / count.
 *  One build gives, all integers, defined bit for bit and independent of the launch:
 *   1. the frontier bit grid [nz][ny][W] in the cast grid's word layout; bits at x >= nx are 0;
 *   2. the voxel indices (the reference's voxel order, :1081) of the frontier cells in ASCENDING order;
 *   3. the records of the non-empty blocks in ASCENDING block index;
 *   4. the counts {n_cells, n_blocks, n_free}; n_free = the cells with free(c).
 *
 *  - dspmap_build_frontiers: enqueued on the handle's stream behind the grid's build and the frame, no synchronisation.
 *  - dspmap_frontier_counts, dspmap_get_frontier_grid: host copies, synchronous.  dspmap_get_frontier_cells / _blocks copy the first
 *    min(cap, n) entries of the list and set *n_out = n, the length of the whole list; out_host may be NULL for cap == 0.
 *  - dspmap_frontier_*_device: the device buffers of the last build, NULL when there is none or it is stale; valid once the handle's
 *    stream has reached the build (the three counts too), until the next build or the handle's destruction.
 *  - arguments, checked before the device is touched, DSPMAP_E_ARG with a text: a NULL handle, a NaN t, max_age < 0, min_unknown outside
 *    1 .. 6, block outside 1 .. DSPMAP_FRONTIER_MAX_BLOCK, flags != 0, a NULL output, cap < 0.  Then, in dspmap_score_views' order: a
 *    sharded handle (slab) is DSPMAP_E_STATE; a stale or never-built grid is DSPMAP_E_STATE with a text naming dspmap_build_cast_grid
 *    (without a usable device this is what a valid call reports: there is no grid without one); a layer without an integration since
 *    its last reset is DSPMAP_E_STATE with a text naming dspmap_known_integrate.  The accessors on a stale or never-built snapshot
 *    are DSPMAP_E_STATE with a text naming dspmap_build_frontiers.
 *  - life cycle.  The result is a snapshot of the grid, of the layer and of the window.  It goes stale with everything that makes the
 *    cast grid stale, with every dspmap_build_cast_grid, dspmap_mask_cast_grid and dspmap_debug_set_cast_grid, with
 *    dspmap_known_integrate, dspmap_known_reset and dspmap_debug_set_known, and with dspmap_set_current_position.
 *  - read-only towards the map, the grid and the known-space layer, beyond the layer's own synchronisation; the captured frame and its
 *    parameter ring are untouched.  The first build allocates one bit grid, V ints for the cell list, one int per grid word and,
 *    per block of the map, two records and a few bytes of scan scratch (these grow when a later build uses a smaller block); all of
 *    it is freed with the device state.  A handle that never builds frontiers allocates nothing.
 *  - dspmap_debug_set_known (test hook): age_host holds V ints in the reference's voxel order, each in [-1, DSPMAP_P_UPDATE_COUNTER -
 *    1]; anything else is DSPMAP_E_ARG; a handle without an accepted frame is DSPMAP_E_STATE.  It synchronises the window, allocates
 *    the store if needed and writes stamp = counter - age (0 for -1) through the toroidal slot mapping, so that dspmap_get_known
 *    returns exactly age_host; the layer counts as integrated.  Synchronous. */
#define DSPMAP_FRONTIER_MAX_BLOCK 32
typedef struct dspmap_frontier_block {
    int block;           /* (Z * nb_y + Y) * nb_x + X */
    int count;           /* frontier cells of the block, >= 1 */
    int sum_x, sum_y, sum_z;   /* sums of their voxel indices per axis */
    int unknown_faces;   /* sum of their u */
} dspmap_frontier_block;
int dspmap_build_frontiers(dspmap_t* m, float t, int max_age, int min_unknown, int block, int flags /* must be 0 */);
int dspmap_frontier_counts(dspmap_t* m, long long out[3]);                       /* {n_cells, n_blocks, n_free}; synchronous */
int dspmap_get_frontier_grid(dspmap_t* m, unsigned long long* out_host);         /* nz * ny * W words; synchronous */
int dspmap_get_frontier_cells(dspmap_t* m, int cap, int* out_host, int* n_out);
int dspmap_get_frontier_blocks(dspmap_t* m, int cap, dspmap_frontier_block* out_host, int* n_out);
const unsigned long long* dspmap_frontier_grid_device(dspmap_t* m);
const int* dspmap_frontier_cells_device(dspmap_t* m);
const dspmap_frontier_block* dspmap_frontier_blocks_device(dspmap_t* m);
const long long* dspmap_frontier_counts_device(dspmap_t* m);
int dspmap_debug_set_known(dspmap_t* m, const int* age_host);

/* ---- objects: the connected components of one layer of the cast grid, each with its box, the sums behind its centroid, and the mass
 * and momentum the filter holds in its cells (no counterpart in the reference).  "There are five obstacles, this one is 0.6 x 0.4 x 1.7 m,
 * centred here, moving at (0.8, -0.1) m/s" is the input of every MPC or velocity-obstacle planner, and the one product of this map that
 * a static occupancy grid cannot give: the filter estimates a mean velocity per voxel (voxels_objects_number[v][1..3],
 * dspmap_get_results), this groups the voxels.  One layer, integers only, no tracking across frames.  An extension beside the frame,
 * like the sections above: the frame path, its launch chain, the captured graph and the parameter ring do not know about it.
 *
 *  Input: the grid of the last dspmap_build_cast_grid EXACTLY AS IT IS (inflated, masked or replaced through
 *  dspmap_debug_set_cast_grid).  t selects ONE layer as for dspmap_build_frontiers: layer 0 for t < 0 or a map without horizons, else
 *  layer 1 + k(t) with the k(t) of dspmap_query_occupancy.
 *  Components: two cells with set bits are adjacent under connectivity 6 when they share a face, under 26 when they share a face, an edge
 *  or a corner.  Cells outside the map do not exist.  The objects are the connected components of the set cells; the label of a
 *  component is the smallest voxel index (the reference's voxel order, :1081) among its cells.
 *  Record: dspmap_object, 88 bytes, all integers -- the label, count = its cells, the box min / max per axis in voxel indices
 *  (inclusive), sum_x, sum_y, sum_z = the sums of its cells' voxel indices per axis, and mass_q, mom_q[3]: mass and momentum in units
 *  of 2^-20, summed over the object's cells from the CURRENT result grid, bit for bit what dspmap_get_results returns, in fixed point so
 *  that the order of arrival cannot matter.  Every named operation is rounded to fp32 on its own.  With w = res[v][0], u_a = res[v][1 + a]:
 *   - a cell contributes to mass_q iff w is finite and 0 < w < 4096: (long long)fl(w * 1048576.0f), the C cast, truncating (the product
 *     is exact);
 *   - the same cell contributes to mom_q[a] iff u_a is finite and |fl(w * u_a)| < 4096: (long long)fl(fl(w * u_a) * 1048576.0f);
 *   - every other cell contributes 0.
 *  A contribution is below 2^32 in magnitude and a map has fewer than 2^31 cells (dspmap_create's limit), so every sum stays below 2^63;
 *  the index sums stay below 2^31 * 2^10.  For a predicted layer (t >= 0) the two sums still say what the filter holds in that region NOW:
 *  the cells are those of the predicted layer, mass and velocity those of the current result grid.  The host derives centroid = sum /
 *  count (a mean voxel index is the centre of that voxel) and velocity = mom_q / mass_q.
 *  One build gives, all integers, defined bit for bit and independent of the launch:
 *   1. the records of the components with count >= min_cells in ASCENDING label; the first max_objects of them are kept, the counts
 *      still report all of them;
 *   2. a label grid of V ints in the reference's voxel order: the ordinal of the voxel's record in that list -- an ordinal >= max_objects
 *      included --, -1 for a clear bit or a component below min_cells;
 *   3. the counts {n_objects, n_components, n_occupied}: the components with count >= min_cells, all components, the set bits of the layer.
 *
 *  - dspmap_build_objects: enqueued on the handle's stream behind the grid's build and the frame, no synchronisation.
 *  - dspmap_object_counts, dspmap_get_object_labels: host copies, synchronous.  dspmap_get_objects copies the first min(cap, n) records
 *    and sets *n_out = n, the records the build kept (min(n_objects, max_objects)); out_host may be NULL for cap == 0 (the convention of
 *    dspmap_get_frontier_cells).
 *  - dspmap_objects_device, dspmap_object_labels_device, dspmap_object_counts_device: the device buffers of the last build, NULL when
 *    there is none or it is stale; valid once the handle's stream has reached the build, until the next build or the handle's
 *    destruction.  The counts buffer holds a fourth word behind the three counts: 0, or why the labelling gave up (below).
 *  - dspmap_query_objects*: the label-grid entry of the voxel that holds the sample (dspmap_point_voxel_index's expression); samples,
 *    frame convention and DSPMAP_QUERY_WORLD as in dspmap_query_known; t is ignored.  -1 outside the map or for a NaN coordinate.  The
 *    _device variant only enqueues.
 *  - arguments, checked before the device is touched and in this order, DSPMAP_E_ARG with a text: a NULL handle, a NaN t, connectivity
 *    not 6 or 26, min_cells < 1, max_objects outside [1, 2^20], flags != 0; a NULL output, cap < 0, n < 0, flags other than
 *    DSPMAP_QUERY_WORLD.  Then a sharded handle (slab) is DSPMAP_E_STATE (components cross slabs); then a stale or never-built grid is
 *    DSPMAP_E_STATE with a text naming dspmap_build_cast_grid.  Accessors and queries without a valid build are DSPMAP_E_STATE with a
 *    text naming dspmap_build_objects.
 *  - the labelling is a union-find on labels that only ever decrease, in launches of its own; no kernel waits for another workgroup and
 *    every loop has a trip bound, so it cannot hang.  Should a bound ever run out, the build records it and the synchronous accessors
 *    return DSPMAP_E_DEVICE.
 *  - life cycle.  The result is a snapshot of the map and of the grid.  It goes stale with everything that makes the cast grid stale and
 *    with every dspmap_build_cast_grid, dspmap_mask_cast_grid and dspmap_debug_set_cast_grid -- not with builds of arrival fields,
 *    distance fields, forecasts or frontiers, not with the known-space calls, not with dspmap_set_current_position.
 *  - read-only towards the map and the grid; the captured frame and its parameter ring are untouched.  The first build allocates three
 *    arrays of V ints, min(max_objects, V) records (more when a later build asks for more) and a few bytes of scan scratch per 256
 *    voxels; all of it is freed with the device state.  A handle that never builds objects allocates nothing. */
typedef struct dspmap_object {
    int label;                        /* smallest voxel index of the component */
    int count;                        /* its cells, >= min_cells */
    int min_x, max_x, min_y, max_y, min_z, max_z;   /* box in voxel indices, inclusive */
    long long sum_x, sum_y, sum_z;    /* sums of voxel indices per axis */
    long long mass_q;                 /* units of 2^-20 */
    long long mom_q[3];               /* units of 2^-20 m/s */
} dspmap_object;
int dspmap_build_objects(dspmap_t* m, float t, int connectivity, int min_cells, int max_objects, int flags /* must be 0 */);
int dspmap_object_counts(dspmap_t* m, long long out[3]);                  /* {n_objects, n_components, n_occupied}; synchronous */
int dspmap_get_objects(dspmap_t* m, int cap, dspmap_object* out_host, int* n_out);
int dspmap_get_object_labels(dspmap_t* m, int* out_host);                 /* V ints; synchronous */
const dspmap_object* dspmap_objects_device(dspmap_t* m);
const int* dspmap_object_labels_device(dspmap_t* m);
const long long* dspmap_object_counts_device(dspmap_t* m);
int dspmap_query_objects(dspmap_t* m, int n, const dspmap_query* q_host, int flags, int* ordinal_out_host);
int dspmap_query_objects_device(dspmap_t* m, int n, const dspmap_query* q_dev, int flags, int* ordinal_out_dev);

/* ---- tracks: the objects of consecutive builds associated by voxel overlap -- ids that persist, an age, a parent for what split off (no
 * counterpart in the reference).  Every dspmap_build_objects numbers the obstacles anew; a planner filters a per-obstacle state over time
 * and needs "obstacle 17 is the one I avoided a moment ago, it has existed for 40 frames, and it just split off obstacle 9".  Like the
 * known-space layer this is persistent state beside the frame, not a snapshot: it lives through frames, and the frame path does not know
 * about it.  After update -> dspmap_build_cast_grid -> dspmap_build_objects the caller calls dspmap_track_update(dt, ...): it
 * associates the objects of the valid build with those the previous update saw and yields one dspmap_track per record, tracks[i]
 * belonging to objects[i].  Integers throughout but the predicted shift, whose double operations are each rounded on their own: the
 * update is defined bit for bit and independent of the launch.  Only enqueued on the handle's stream, no synchronisation, no host read.
 *
 *  Input: records, label grid and counts of the valid dspmap_build_objects, K_now = min(n_objects, max_objects) read on the device; the
 *  tracker's own copy of the same three from the previous update, K_prev, with the previous tracks; and the window: k0[a], the world
 *  lattice index of map voxel 0 on axis a, from the current position by the known-space layer's expression (above), dk0 = k0_now - k0_prev.
 *  Fresh start: without a previous state (first update, after a reset, a new state or a void update), or with |dk0[a]| >= n[a] on some
 *  axis, nothing is associated: every object is born, the previous tracks all end.
 *  Predicted shift per previous track j, from its record: with mass_q > 0, per axis v = (double)mom_q[a] / (double)mass_q,
 *  d = v * (double)dt, e = d / (double)res, p = floor(e + 0.5), then p clamped to [-max_shift, max_shift] while still a double; with
 *  mass_q <= 0, p = 0.  shift_j[a] = (int)p - dk0[a].  dt = 0 is pure overlap.
 *  Overlap: every cell c of the previous label grid whose ordinal is j < K_prev looks at c' = c + shift_j; if c' lies inside the map and
 *  the current label grid holds o with 0 <= o < K_now there, n(j, o) += 1.  Ordinals >= K on either side and -1 contribute nothing.
 *  Association: bj(o) = the j with the largest n(j, o) > 0, ties to the smaller j; bo(j) = the o with the largest n(j, o) > 0, ties to
 *  the smaller o; o is matched to j iff bj(o) = j, bo(j) = o and n(j, o) >= min_overlap.
 *  A matched track: id, parent and born_seq of track j; age = age_j + 1; prev_ordinal = j; overlap = n(j, o); shift_* = shift_j;
 *  prev_count = count_j; prev_sum_a = sum_a,j - count_j * dk0[a], the previous index sums in the CURRENT window's voxel indices, so that
 *  sum / count - prev_sum / prev_count is the centroid's displacement in voxels.
 *  A born track: id = next_id + r, r its rank among the unmatched objects in ascending ordinal; parent = the id of track bj(o) if bj(o)
 *  exists (what a split leaves behind names its parent this way), else -1; age = 0; born_seq = the number of updates enqueued since the
 *  last reset before this one (the first is 0; a void update counts); prev_ordinal = -1; overlap = n(bj(o), o) or 0; shifts, prev_count
 *  and prev_sum_* 0.  Then next_id += the number born.  Ids start at 0 after a reset.
 *  Counts, long long[6]: {n_tracks, n_matched, n_born, n_ended, n_pairs, next_id}; n_ended = the previous tracks without a match, n_pairs
 *  = the distinct (j, o) with n > 0.  The device buffer holds a seventh word: 0, or 1 when the pair table was full.
 *  Pair table: n(j, o) lives in an open-addressing table of max_pairs slots -- 0 selects 8 x the record capacity of the objects, at least
 *  1024; any value is rounded up to a power of two, at most 2^24.  Probing is bounded by the table size.  If an insert finds no slot --
 *  exactly when the distinct pairs exceed the slots -- the update is VOID: the fault word is 1, the counts are 0 but next_id, which is
 *  unchanged, the stored previous state is emptied on the device (the following update starts fresh), and the synchronous accessors
 *  return DSPMAP_E_DEVICE with a text naming max_pairs.  An ordinary, reported outcome of a capacity argument, like the exhausted bound
 *  of dspmap_build_objects.
 *  flags: DSPMAP_TRACK_PER_CELL makes one table insert per contributing cell instead of one per run of equal pairs along x; the same
 *  bytes, for measurements and tests.
 *
 *  - dspmap_track_reset: everything forgotten, ids from 0 again; dspmap_clear_state and dspmap_load_checkpoint do the same.
 *  - dspmap_track_counts: synchronous.  dspmap_get_tracks: the conventions of dspmap_get_objects, *n_out = n_tracks.
 *  - dspmap_tracks_device, dspmap_track_counts_device: the device buffers of the last update (the track array changes with every
 *    update), NULL without one; valid once the handle's stream has reached the update, until the next update or reset.
 *  - checks, in this order.  DSPMAP_E_ARG with a text, before the device is touched: a NULL handle, dt NaN, negative or infinite,
 *    min_overlap < 1, max_shift outside [0, 64], max_pairs < 0, unknown flags; a NULL output, cap < 0.  Then a sharded handle (slab) is
 *    DSPMAP_E_STATE; then no valid build of objects is DSPMAP_E_STATE with a text naming dspmap_build_objects; then a position the
 *    known-space window refuses.  Accessors without an update are DSPMAP_E_STATE with a text naming dspmap_track_update.
 *  - life cycle.  The tracks of the last update stay readable through frames, until the next update or reset; only their pairing with
 *    objects[i] depends on that build.  Nothing that makes a snapshot stale touches them, and an update makes no snapshot stale.
 *  - a handle that never tracks allocates nothing.  The first update allocates a copy of the label grid (V ints), copies of the records
 *    and counts, two track arrays (swapped, not copied), the per-track shifts, the two best arrays, the pair table and a little scan
 *    scratch; all of it is freed with the device state. */
#define DSPMAP_TRACK_PER_CELL 1
typedef struct dspmap_track {
    long long id;                     /* persists while the track is matched */
    long long parent;                 /* id of the track it was born from (a split), or -1 */
    long long prev_sum_x, prev_sum_y, prev_sum_z;   /* the previous index sums in the current window's voxel indices */
    int prev_count;                   /* the previous record's cells, 0 for a born track */
    int prev_ordinal;                 /* its ordinal in the previous build, -1 for a born track */
    int age;                          /* updates since it was born */
    int born_seq;                     /* sequence number of the update it was born in */
    int overlap;                      /* n(j, o) of the match, or of the best previous track of a born one */
    int shift_x, shift_y, shift_z;    /* shift_j of the match */
} dspmap_track;
int dspmap_track_update(dspmap_t* m, float dt, int min_overlap, int max_shift, int max_pairs, int flags);
int dspmap_track_reset(dspmap_t* m);
int dspmap_track_counts(dspmap_t* m, long long out[6]);                   /* synchronous */
int dspmap_get_tracks(dspmap_t* m, int cap, dspmap_track* out_host, int* n_out);
const dspmap_track* dspmap_tracks_device(dspmap_t* m);
const long long* dspmap_track_counts_device(dspmap_t* m);

/* getVoxelPositionFromIndexPublic :1556-1572 / getPointVoxelsIndexPublic :1574-1584 (host math) */
void dspmap_voxel_center(const dspmap_t* m, int index, float* px, float* py, float* pz);
int dspmap_point_voxel_index(const dspmap_t* m, float px, float py, float pz, int* index);

/* ---- sizes ---- */
int dspmap_voxel_num(const dspmap_t* m);        /* global VOXEL_NUM :62 */
int dspmap_local_voxel_num(const dspmap_t* m);  /* voxels in this handle's slab */
int dspmap_local_voxel_base(const dspmap_t* m); /* global index of the slab's first voxel (0 for an unsharded map) */
int dspmap_slots_per_voxel(const dspmap_t* m);  /* SAFE_PARTICLE_NUM_VOXEL :65 */
int dspmap_pyramid_num(const dspmap_t* m);      /* observation_pyramid_num :60 */
int dspmap_pyramid_capacity(const dspmap_t* m); /* SAFE_PARTICLE_NUM_PYRAMID :66 */
int dspmap_get_counters(dspmap_t* m, dspmap_counters* out);

/* per-stage device timing (HIP events on the handle's stream around each kernel group).
 * Off by default; when on, every update records events and the elapsed times accumulate.
 * Stages: 0 setup+binning, 1 predict, 2 claim(movers), 3 Ck partial, 4 weight update,
 *         5 Ck sum (birth normaliser), 6 birth, 7 occupancy+resample. */
#define DSPMAP_N_STAGES 8
int dspmap_set_profiling(dspmap_t* m, int on);
int dspmap_get_stage_ms(dspmap_t* m, float ms_sum_out[DSPMAP_N_STAGES], int* n_frames_out); /* sums since enabling; syncs */
/* what one event bracket adds to the kernel inside it (record cost + launch gaps), calibrated when profiling is switched on with a
 * kernel of known duration: stage time - this = the kernel's own duration for the stages that are one launch */
int dspmap_get_event_overhead_ms(dspmap_t* m, float* ms_out);

/* profiling aid: streams the six particle field arrays once with the sweeps' access pattern
 * (4 B per lane, 256 B per wave) -- mode 0 reads them (known byte count = 6*4*capacity), mode 1
 * rewrites px in place -- to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE for this pattern. */
int dspmap_debug_stream(dspmap_t* m, int mode, long long* bytes_out);
/* profiling aid: the bare memory skeleton of the prediction sweep -- one workgroup per 64-voxel tile, the first `rows` slot
 * rows of every tile, nothing computed -- timed with events over `reps` launches: what the memory system sustains for
 * this access pattern.  what: bit 0 read positions (12 B), bit 1 read velocities (8 B), bit 2 read weights (4 B),
 * bit 3 write positions back (12 B); rows_per_batch = rows a wave keeps in flight.  *bytes_out = bytes per launch. */
int dspmap_debug_sweep_probe(dspmap_t* m, int what, int rows, int rows_per_batch, int reps, float* ms_out, long long* bytes_out);
/* diagnostics: out[t] = 1 if a particle inside 64-voxel tile t could lie in the field of view of the last frame
 * (the conservative box test behind DSPMAP_P_PLACE_SPLIT_TILES); returns the number of tiles or an error */
int dspmap_debug_tile_view(dspmap_t* m, int* out, int cap);
/* diagnostics: the number of 64-voxel tiles of this handle's storage, and the tile each of n voxels (GLOBAL indices of the reference, :1081) lives
 * in (-1: not in this handle's slab).  A tile is a run of 64 voxel indices or a cube of 4 x 4 x 4 voxels (DSPMAP_P_TILING) */
int dspmap_debug_tile_count(dspmap_t* m);
int dspmap_debug_tile_of_voxels(dspmap_t* m, int n, const int* voxel_global_host, int* tile_out_host);
/* diagnostics: out[t] = the "somebody moves" flag of 64-voxel tile t: 0 = every live particle of the tile had velocity (0, 0)
 * when k_predict last swept it and nothing with a velocity has arrived or been born there since -- the sweeps of such a tile do
 * not fetch its velocity rows (k_predict).  Returns the number of tiles or an error */
int dspmap_debug_tile_moving(dspmap_t* m, int* out, int cap);
/* diagnostics: which kernels the last resampling stage ran and which path the future-status contributions took:
 * out[0] = bit 0: four-waves-per-tile resampler; bits 1-2: rollout 0 inside the resampler, 1 k_rollout without LDS windows,
 * 2 k_rollout with LDS windows, 3 none; out[1] / out[2] = contributions k_rollout sent through its windows / as single atomics */
int dspmap_debug_rollout_paths(dspmap_t* m, long long out[3]);
/* diagnostics: the work items the last weight update (a frame's or dspmap_stage_update's) was split into: out[0] = items of k_ck_partial
 * (chunks of out[2] particles of the lists of pyramids with an observation in their neighbourhood), out[1] = items of k_weight
 * (256 / lanes-per-particle particles each, at least one per pyramid), out[2] = particles per k_ck_partial item (32 or 64).  Syncs */
int dspmap_debug_pair_items(dspmap_t* m, int out[3]);
/* which instantiation of k_weight the last weight update launched: 1 = every pair of a neighbourhood evaluated and the far ones masked,
 * 2 = only the observations within range of the item staged and far pairs branched over (maps whose corner is farther than 12 cull
 * radii), 0 = none yet.  Both add the same terms (DSPMAP_P_PAIR_CULL_SIGMAS) */
int dspmap_debug_weight_variant(dspmap_t* m);
/* how the last frame (or dspmap_stage_update) gave its pair kernels their work (DSPMAP_P_PAIR_PREPARE): 1 = k_pyr_prepare sorted and cut the
 * pyramid lists and wrote the item lists, 2 = self-mapped pair kernels on the lists as registered, 0 = none yet */
int dspmap_debug_pair_path(dspmap_t* m);
/* diagnostics: the window plan k_rollout gets on this handle (a function of the configuration and the storage order alone; no device
 * needed): halo_out[t] = rows of the grid horizon t's LDS window reaches beyond its group of tiles, either side (-1 past the last
 * horizon), *lds_cells_out = 32-bit cells of all windows together (may be NULL).  All halos 0 = the collapsed plan of a grid too wide
 * for one-row halos: every window is the group itself.  Returns the number of horizons or an error */
int dspmap_debug_rollout_plan(dspmap_t* m, int halo_out[DSPMAP_MAX_PRED_TIMES], int* lds_cells_out);
/* diagnostics of DSPMAP_P_ESTIMATOR_QUEUE: out[0] = frames of this handle whose velocity estimator ran on a queue of its own, out[1] / out[2] = the
 * two hand-over words (ring position + 1 of the last frame whose birth stage has ended / whose birth cloud the estimator has finished),
 * out[3] = nonzero if a cross-queue wait ever gave up, out[4] = frames whose first birth kernel found the birth cloud unfinished (its workgroup 0
 * waited, the other workgroups left their shares to it), out[5] = shares it did for them */
int dspmap_debug_estimator_queue(dspmap_t* m, long long out[6]);
/* where the last frame with the device velocity estimator ran it: 1 = on a stream of its own (DSPMAP_P_ESTIMATOR_QUEUE), 2 = as a forked branch of the
 * captured frame because no stream apart from the main stream's hardware queue was found (the fallback), 3 = as a forked branch (switched off, a map
 * that splits its placement, or after a cross-queue wait gave up), 0 = no such frame yet.  Test hooks, read at dspmap_create: DSPMAP_XQ_FORCE=shared
 * (every candidate stream counts as sharing the queue: the fallback runs), DSPMAP_XQ_FORCE=apart (fail instead of falling back) */
int dspmap_debug_estimator_path(dspmap_t* m);
/* diagnostics of DSPMAP_P_FRAME_BRANCHES: out[0] = frames of this handle that ran as two branches, out[1] / out[2] = tiles of class Q (a newborn of
 * the last such frame could land there) / P (a particle could reach a Q tile), out[3] = tiles of the map, out[4] = the largest speed any particle
 * of the map was ever given, mm/s (what sizes P) */
int dspmap_debug_frame_branches(dspmap_t* m, long long out[5]);
/* frames of this handle whose resampling stage ran as two launches (DSPMAP_P_RESAMPLE_SPLIT) */
long long dspmap_debug_resample_split_frames(dspmap_t* m);
/* frames of this handle that were queued as plain launches with their parameter block in the pinned ring: every device-resident frame under
 * DSPMAP_P_USE_GRAPH = 2, the small maps' single-chain frames (and two-branch frames) under the default */
long long dspmap_debug_plain_frames(dspmap_t* m);
/* test hooks of dspmap_mgpu_comm_init_from_env's rendezvous file (no device, no RCCL): what rank 0 publishes / what a rank != 0
 * waits for (this launch's nonce: DSPMAP_RDZV_NONCE or TORCHELASTIC_RUN_ID + the parent's pid).  1 = written / found, 0 = not */
int dspmap_debug_rdzv_publish(const char* path, const char id[128]);
int dspmap_debug_rdzv_wait(const char* path, int timeout_ms, char id_out[128]);

/* ---- state access (the reference's equivalent is direct access to its
 * file-scope arrays, dsp_dynamic.h:116).  A record is 8 floats
 * {flag, vx, vy, vz, px, py, pz, weight} (:114-115 minus the dead update_time).
 * `voxel` is the GLOBAL voxel index; slot < 0 = first free slot (:1184-1185). ---- */
int dspmap_clear_state(dspmap_t* m);
int dspmap_import_state(dspmap_t* m, int n, const int* voxel_host, const int* slot_host, const float* rec8_host);
int dspmap_export_state(dspmap_t* m, int cap, int* voxel_out_host, int* slot_out_host, float* rec8_out_host, int* n_out);
/* ---- binary checkpoint / restore (the reference has none).  Saves every live particle with its
 * slot, the function statics of update() and of the birth stage, the table cursors, the result grid and the future
 * accumulators; the random tables come from the configuration's seed (or are re-injected by the caller).  Loading
 * requires a handle created with the same configuration.  The host velocity estimator's previous clusters are not
 * saved: the first frame after a restore matches no cluster, like the first frame of a run.  Nor is the cloud of the
 * last view that had points: a frame with an empty view re-uses it for its births (:1379-1381), so a restored handle
 * whose FIRST frames have an empty view gives birth to nothing until a frame with points has come.  The filter
 * parameters of dspmap_set_param are saved and restored, DSPMAP_P_PAIR_CULL_SIGMAS excepted (the loading handle's). */
int dspmap_save_checkpoint(dspmap_t* m, const char* path);
int dspmap_load_checkpoint(dspmap_t* m, const char* path);
/* ---- caller-side pre-processing on the device (next to the hot path; reference src/map_sim_example.cpp:309-336)
 * points_dev: n points, xyz first, stride_floats floats apart, device memory, in the frame the sensor driver
 * delivers (swap_axes = 1: camera optical frame, mapped x = z, y = -x, z = -y like :321-323; 0: already x forward).
 * Voxel-grid centroid filter with leaf size `leaf` (pcl::VoxelGrid, :313-317), crop to the open map box (:325),
 * at most max_points points in the filter's output order (:332) -> out_dev (max_points x 3 floats, device memory,
 * ready for dspmap_update_device).  *n_out = points written, *n_leaves_out (optional) = occupied leaves that touch
 * the map box.  Non-finite points are ignored (PCL does the same for non-dense clouds).  Only leaves touching the
 * map box are accumulated (the others cannot survive the crop), so the cost does not depend on far returns;
 * refuses leaf sizes that put more than 2^27 leaves into the map box. */
int dspmap_preprocess_cloud(dspmap_t* m, int n, const float* points_dev, int stride_floats, float leaf, int swap_axes,
                            int max_points, float* out_dev, int* n_out, int* n_leaves_out);

/* ---- depth images straight to the map (what a node with a depth topic owns is a 16UC1 / 32FC1 image, not a cloud).
 * One kernel reads the image, back-projects every kept pixel in registers and accumulates the voxel-grid filter's leaf sums; the 12 B per
 * pixel cloud never exists in memory.  Per kept pixel (u = column, v = row), every operation rounded to fp32 on its own:
 *     d = fl((float)raw * depth_scale)                                   (DSPMAP_DEPTH_F32: raw is the float itself)
 *     X = fl(fl(fl((float)u - cx) * d) / fx)   Y = fl(fl(fl((float)v - cy) * d) / fy)   Z = d        camera optical frame
 * A pixel is kept iff it is a return (format) and min_depth <= d <= max_depth.  Leaf membership, the leaf lattice over the map box, the
 * output order, the axis swap x = Z, y = -X, z = -Y, the open-box crop and the cap are those of dspmap_preprocess_cloud(swap_axes = 1)
 * applied to (X, Y, Z) (a pixel whose X, Y or Z is not finite is ignored like a non-finite point).  Only the CENTROID differs: each
 * coordinate is accumulated per leaf as the 64-bit integer llrint((double)p * 2^20) (ties to even) and the centroid is
 * (float)(((double)S / (double)count) * 2^-20).  Integer sums do not depend on the order of the additions: the filtered cloud is the same
 * bits on every run, launch shape and pixel order.
 * Arguments are checked before the device is touched: a NULL handle / camera / image, width, height or pixel_step < 1 (or a side or a
 * pixel_step above 2^24: a larger step would overflow the pixel column of the tile's unused lanes), a row stride smaller than a row or not a multiple of the element size, an unknown format, non-finite or non-positive fx,
 * fy, depth_scale, non-finite cx, cy, min_depth > max_depth or a NaN among them, leaf <= 0, max_points < 0 (or NULL outputs / pose) are
 * DSPMAP_E_ARG with a text; without a usable device a valid call is DSPMAP_E_DEVICE. */
#define DSPMAP_DEPTH_U16 0   /* raw units, value 0 = no return (RealSense / ROS 16UC1) */
#define DSPMAP_DEPTH_F32 1   /* raw floats; NaN, +-inf and values <= 0 = no return (ROS 32FC1) */
typedef struct dspmap_camera {
    int width, height;
    int row_stride_bytes;       /* 0 = packed */
    int format;                 /* DSPMAP_DEPTH_* */
    float fx, fy, cx, cy;       /* pinhole intrinsics, pixels */
    float depth_scale;          /* metres per raw unit (0.001 for millimetres, 1 for 32FC1) */
    float min_depth, max_depth; /* metres; a pixel is kept iff min_depth <= d <= max_depth */
    int pixel_step;             /* use rows and columns 0, step, 2*step, ...; 1 = every pixel, at most 2^24 */
} dspmap_camera;
/* depth image in device memory -> filtered cloud in device memory; same outputs and the same synchronous contract as
 * dspmap_preprocess_cloud(swap_axes = 1); *n_valid_out (optional) = pixels that passed the validity and range test */
int dspmap_preprocess_depth(dspmap_t* m, const dspmap_camera* cam, const void* depth_dev, float leaf, int max_points,
                            float* out_dev, int* n_out, int* n_leaves_out, int* n_valid_out);
/* the whole frame from one image: ingest as above into a buffer the handle owns, then exactly dspmap_update_device(n_out, that
 * buffer, 0, NULL, ...).  1 / 0 / negative like dspmap_update; a rejected frame (0) leaves the map state untouched: the gate of
 * dspmap_update (quaternion, |dp| > 10 m, dt outside [0, 10] s) is evaluated before any ingest work is queued.  The frame itself is
 * asynchronous like dspmap_update_device; the call waits for the ingest (one 12-byte read of the point count, which the frame's
 * parameter block takes from the host). */
int dspmap_update_depth_device(dspmap_t* m, const dspmap_camera* cam, const void* depth_dev, float leaf, int max_points,
                               const float sensor_pos[3], double time_stamp_second, const float quat_wxyz[4]);
/* the same with the image in host memory (one pinned staging copy + H2D of the IMAGE, not of a cloud) */
int dspmap_update_depth(dspmap_t* m, const dspmap_camera* cam, const void* depth_host, float leaf, int max_points,
                        const float sensor_pos[3], double time_stamp_second, const float quat_wxyz[4]);

/* addRandomParticles :594-624 (constructor pre-fill); uses the rand table */
int dspmap_add_random_particles(dspmap_t* m, int n, float weight);
/* benchmark fill: every voxel gets `per_voxel` zero-velocity particles,
 * uniform in-voxel positions, given weight; generated on device from `seed`. */
int dspmap_seed_uniform(dspmap_t* m, int per_voxel, float weight, unsigned seed);
/* same fill with velocities uniform in [-vmax, vmax] (benchmark of the future-status rollout) */
int dspmap_seed_uniform_moving(dspmap_t* m, int per_voxel, float weight, unsigned seed, float vmax);

/* ---- single stages on the current state (test hooks; the reference's
 * stages are private members made reachable the same way by its own author
 * for mapAddNewBornParticlesByObservation, :795-796) ---- */
int dspmap_stage_bin_points(dspmap_t* m, int n, int stride, const float* pts_host,
                            float qw, float qx, float qy, float qz);                  /* :220-293 */
int dspmap_set_current_position(dspmap_t* m, float x, float y, float z);             /* :213-215 */
int dspmap_stage_predict(dspmap_t* m, float odom_dx, float odom_dy, float odom_dz, float dt); /* mapPrediction :627 */
int dspmap_stage_update(dspmap_t* m);                                                /* mapUpdate :704 */
int dspmap_stage_birth(dspmap_t* m);                                                 /* mapAddNewBornParticlesByObservation :796 */
int dspmap_stage_resample(dspmap_t* m);                                              /* mapOccupancyCalculationAndResample :924 */
/* observation bins after binning / update: xyz+Ck+len per stored obs (:497-501,514-515) */
int dspmap_get_observations(dspmap_t* m, float* obs_out_host /* [NP][100][5] */, int* count_out_host /* [NP] */,
                            float* max_len_out_host /* [NP] */, float* expected_newborn_out);
int dspmap_set_expected_newborn(dspmap_t* m, float v);
/* particles registered per pyramid by the last prediction (size of each pyramids_in_fov list, :124) */
int dspmap_get_pyramid_counts(dspmap_t* m, int* count_out_host /* [NP] */);
/* particles the last prediction tried to register per pyramid, before the cut to SAFE_PARTICLE_NUM_PYRAMID (this rank's
 * share on a sharded map): list length + the particles turned away (-2, :1256-1259) */
int dspmap_get_pyramid_candidates(dspmap_t* m, int* count_out_host /* [NP] */);

/* ---- multi-GPU split-phase frame (Z-slab sharding; the single-process reference has no
 * counterpart).  One process per GPU owns the voxel layers [z_lo, z_hi) (dspmap_config).  Every
 * rank is fed the same cloud and pose; per frame the caller runs
 *     begin -> export(+1), export(-1) [or export_both] -> (place_interior) -> [send to rank+1 / rank-1] -> import
 *           -> ck_partial (places the movers, imported ones included, then the Ck pass) -> [all-reduce SUM over the bound Ck buffer]
 *           -> weights_and_split -> [all-reduce MAX over the bound n_static buffer]
 *           -> finish
 * and issues the collectives itself (RCCL through torch.distributed).  What crosses slabs:
 *  (1) particles whose new voxel lies in another slab after prediction (vz == 0, so only the
 *      ego-motion's z component moves particles across layers, dsp_dynamic.h:661-667);
 *  (2) the per-observation sums Ck, because pyramids cut across slabs (:709-735);
 *  (3) n_static of each birth source, known only to the rank owning the source's voxel (:827-866).
 * Records are 8 floats {global voxel index (int bits), vx, vy, px, py, pz, w, source key (int bits)}: the key
 * (source voxel * slots + slot) orders the arrivals of a voxel as the reference's sequential sweep would serve them;
 * imported records are placed together with the slab's own movers (the placement pass runs after the import), so
 * a sharded map fills exactly the slots of the unsharded one.
 * The Ck buffer holds 64-bit fixed-point sums (units of 2^-34): all-reduce it as int64.  Integer addition is
 * associative, so a sharded frame computes exactly the Ck of the unsharded one and frames are reproducible. */
int dspmap_mgpu_bind(dspmap_t* m, long long* ck_dev /* [NP*100] int64 */, int* nstatic_dev, int nstatic_cap);
/* optional, between the exports and the imports: places the movers of the slab's interior (the tiles no record of a
 * neighbour can reach this frame) so that the GPU works while the caller sizes the exchange on the host */
int dspmap_mgpu_place_interior(dspmap_t* m);
int dspmap_mgpu_begin(dspmap_t* m, int n_points, const float* points_dev, int n_birth,
                      const dspmap_vpoint* birth_dev, const float sensor_pos[3],
                      double time_stamp_second, const float quat_wxyz[4]);   /* 1 / 0 like dspmap_update */
int dspmap_mgpu_export(dspmap_t* m, int dir /* +1 through z_hi, -1 through z_lo */, float* rec_dev_out,
                       int cap, int* n_out);                                 /* synchronises */
/* stream-ordered variant of the two exports: no host synchronisation; counts_dev[0] = records written to
 * up_dev_out, counts_dev[1] = to down_dev_out (device memory).  A count above `cap` means the buffer was too small
 * (the surplus particles are lost): the caller must check after reading the counts, then report them with
 * dspmap_mgpu_set_export_counts (statistics only). */
int dspmap_mgpu_export_both(dspmap_t* m, float* up_dev_out, float* down_dev_out, int cap, int* counts_dev);
int dspmap_mgpu_set_export_counts(dspmap_t* m, int n_up, int n_down);
int dspmap_mgpu_import(dspmap_t* m, int n, const float* rec_dev);
int dspmap_mgpu_ck_partial(dspmap_t* m);
int dspmap_mgpu_weights_and_split(dspmap_t* m);
int dspmap_mgpu_finish(dspmap_t* m);

/* ---- the same frame driven from C++ (dspmap_dist.hip): one call per frame and rank, the collectives are issued by the
 * library on its own stream through RCCL (dlopen of librccl.so at communicator set-up), no host synchronisation inside a
 * frame.  Exchange of the boundary particles = fixed-size ncclSend / ncclRecv pairs with rank +- 1 whose first record
 * is a header carrying the record count; the size is the largest export of an earlier frame (all ranks) + 50 % + 1024,
 * agreed through one extra slot of the n_static all-reduce (MAX); particles that cross more than one slab are forwarded
 * in further rounds.  Ck: ncclAllReduce(SUM, int64); n_static: ncclAllReduce(MAX, int32).
 *   rank 0:      dspmap_mgpu_get_unique_id(id)   -> hand `id` to the other ranks (MPI, torch.distributed, a file, ...)
 *   every rank:  dspmap_mgpu_comm_init(m, world, rank, id)       [or dspmap_mgpu_comm_init_from_env: RANK / WORLD_SIZE +
 *                                                                 a rendezvous file, DSPMAP_RDZV_FILE]
 *   per frame:   dspmap_mgpu_update(m, ...)                       1 / 0 like dspmap_update; same cloud and pose on every rank
 * The handle's configuration carries the rank's slab [z_lo, z_hi).  dspmap_mgpu_update returns DSPMAP_E_STATE once, a
 * frame late, if a frame's export did not fit the message (vertical step much larger than the frames before). */
#define DSPMAP_UNIQUE_ID_BYTES 128
int dspmap_mgpu_get_unique_id(char id_out[DSPMAP_UNIQUE_ID_BYTES]);
int dspmap_mgpu_comm_init(dspmap_t* m, int world, int rank, const char id[DSPMAP_UNIQUE_ID_BYTES]);
int dspmap_mgpu_comm_init_from_env(dspmap_t* m);
int dspmap_mgpu_comm_destroy(dspmap_t* m);
int dspmap_mgpu_update(dspmap_t* m, int n_points, const float* points_dev, int n_birth, const dspmap_vpoint* birth_dev,
                       const float sensor_pos[3], double time_stamp_second, const float quat_wxyz[4]);
int dspmap_mgpu_update_host(dspmap_t* m, int point_cloud_num, int size_of_one_point, const float* point_cloud_ptr,
                            float sensor_px, float sensor_py, float sensor_pz, double time_stamp_second,
                            float qw, float qx, float qy, float qz);
int dspmap_mgpu_message_records(const dspmap_t* m);   /* records the next frame's exchange messages carry */
/* the same driver over several slabs inside ONE process (tests, single-GPU debugging): device-to-device copies and small
 * reduction kernels stand in for the collectives; the handles share the first one's stream */
int dspmap_mgpu_group_create(dspmap_t** handles, int n);
int dspmap_mgpu_group_update(dspmap_t** handles, int n, int n_points, const float* points_dev, int n_birth,
                             const dspmap_vpoint* birth_dev, const float sensor_pos[3], double time_stamp_second,
                             const float quat_wxyz[4]);

/* per-slab, per-phase device time of the group's frames (HIP events around every phase of every slab; slab index n = the group's
 * stand-ins for the collectives).  Inside the group every slab has the GPU to itself for the length of its phase -- what its own
 * GPU would spend on it in a one-process-per-GPU run -- so  sum over phases of max over slabs  is the frame's critical path on n GPUs
 * without the transport: the figure bench.py reports as projected_8gpu (a projection; N > 1 has not run on hardware).
 * phases: 0 begin (binning, prediction, estimator, export), 1 exchange + import, 2 placement, 3 list selection (only frames that
 * run it; group level), 4 list preparation + Ck, 5 weights + split, 6 births + resampling + rollout.
 * out: [n + 1][DSPMAP_GROUP_PHASES] summed ms since enabling */
#define DSPMAP_GROUP_PHASES 7
int dspmap_mgpu_group_set_profiling(dspmap_t** handles, int n, int on);
int dspmap_mgpu_group_get_phase_ms(dspmap_t** handles, int n, float* ms_sum_out, int* n_frames_out);

#ifdef __cplusplus
}
#endif
#endif /* DSPMAP_H */
