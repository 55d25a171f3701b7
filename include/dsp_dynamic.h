/*
 * dsp_dynamic.h -- drop-in replacement for g-ch/DSP-map's include/dsp_dynamic.h:
 * the same `class DSPMap` public surface (reference file:line cited per member),
 * forwarding to the MI355X-native library libdspmap_hip.so through the C ABI in
 * dspmap.h.  A caller written against the reference header -- e.g. its
 * src/map_sim_example.cpp -- compiles against this one unchanged and links with
 * -ldspmap_hip.
 *
 * What is kept for source compatibility (all used by src/map_sim_example.cpp):
 *   - the configuration macros MAP_LENGTH_VOXEL_NUM ... PREDICTION_TIMES and the
 *     constants VOXEL_NUM, prediction_future_time[] (:38-47,62); unlike the
 *     reference they can be overridden with -D (the library is sized at run time)
 *   - `using namespace std;` (:35) and the transitive Eigen / PCL includes (:27-31)
 *     when those libraries are installed; without PCL a minimal pcl::PointCloud
 *     is provided so that the header is usable on machines without ROS
 *   - construction during static initialisation is safe (:39 of the example):
 *     no HIP call happens before the first update()
 * New: getFutureStatus() (the name BASELINE.json's north_star uses) and
 * `dspmap_handle()` for callers that want the device-resident views of dspmap.h.
 */
#ifndef DSP_DYNAMIC_H_MI355X
#define DSP_DYNAMIC_H_MI355X

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#if defined(__has_include)
#if __has_include("Eigen/Eigen")
#include "Eigen/Eigen"
#endif
#if __has_include(<pcl/point_types.h>)
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#define DSPMAP_HAVE_PCL 1
#endif
#endif

#include "dspmap.h"

using namespace std;  // the reference header does this (:35) and its example relies on it

#ifndef DSPMAP_HAVE_PCL
namespace pcl {  // minimal containers with the members the DSPMap interface touches
struct PointXYZ { float x = 0, y = 0, z = 0; };
struct PointXYZINormal { float x = 0, y = 0, z = 0, intensity = 0, normal_x = 0, normal_y = 0, normal_z = 0; };
template <typename T>
struct PointCloud {
    std::vector<T> points;
    unsigned width = 0, height = 1;
    void push_back(const T& p) { points.push_back(p); width = (unsigned)points.size(); }
    void clear() { points.clear(); width = 0; }
    size_t size() const { return points.size(); }
    bool empty() const { return points.empty(); }
    T& operator[](size_t i) { return points[i]; }
    const T& operator[](size_t i) const { return points[i]; }
    typename std::vector<T>::iterator begin() { return points.begin(); }
    typename std::vector<T>::iterator end() { return points.end(); }
};
}  // namespace pcl
#endif

/** Parameters for the map (reference :38-47) **/
#ifndef MAP_LENGTH_VOXEL_NUM
#define MAP_LENGTH_VOXEL_NUM 66
#endif
#ifndef MAP_WIDTH_VOXEL_NUM
#define MAP_WIDTH_VOXEL_NUM 66
#endif
#ifndef MAP_HEIGHT_VOXEL_NUM
#define MAP_HEIGHT_VOXEL_NUM 40
#endif
#ifndef VOXEL_RESOLUTION
#define VOXEL_RESOLUTION 0.15
#endif
#ifndef ANGLE_RESOLUTION
#define ANGLE_RESOLUTION 3
#endif
#ifndef MAX_PARTICLE_NUM_VOXEL
#define MAX_PARTICLE_NUM_VOXEL 9
#endif
#ifndef LIMIT_MOVEMENT_IN_XY_PLANE
#define LIMIT_MOVEMENT_IN_XY_PLANE 1
#endif
#ifndef PREDICTION_TIMES
#define PREDICTION_TIMES 6
#define DSPMAP_PREDICTION_TIME_LIST 0.05f, 0.2f, 0.5f, 1.f, 1.5f, 2.f
#elif PREDICTION_TIMES == 1 && !defined(DSPMAP_PREDICTION_TIME_LIST)
#define DSPMAP_PREDICTION_TIME_LIST 0.05f   /* dsp_static.h:46-47 */
#endif
#ifdef DSPMAP_PREDICTION_TIME_LIST
static const float prediction_future_time[PREDICTION_TIMES] = {DSPMAP_PREDICTION_TIME_LIST};
#endif  /* otherwise the including file defines prediction_future_time[PREDICTION_TIMES] before this header */
#if !LIMIT_MOVEMENT_IN_XY_PLANE
#error "libdspmap_hip implements the reference's default LIMIT_MOVEMENT_IN_XY_PLANE 1 (vz == 0)"
#endif

static const int VOXEL_NUM = MAP_LENGTH_VOXEL_NUM * MAP_WIDTH_VOXEL_NUM * MAP_HEIGHT_VOXEL_NUM;  // :62
#ifndef DSPMAP_HALF_FOV_H
#define DSPMAP_HALF_FOV_H 42
#endif
#ifndef DSPMAP_HALF_FOV_V
#define DSPMAP_HALF_FOV_V 24   /* 27 in the reference's two other headers */
#endif
static const int half_fov_h = DSPMAP_HALF_FOV_H;  // :49
static const int half_fov_v = DSPMAP_HALF_FOV_V;  // :50

#ifndef DSPMAP_NO_SAVE_FOLDER_GLOBAL
static string particle_save_folder = ".";  // :55 (one per translation unit here: the reference's non-static global could not be included twice)
#endif

#ifndef DSPMAP_ESTIMATOR_MODE
#define DSPMAP_ESTIMATOR_MODE 2   /* velocityEstimationThread on the device (dspmap_velest.hip); 1 = the host stage.  A sharded map
                                     (-DDSPMAP_WORLD) runs the device estimator on every rank: same cloud, same tagged birth cloud */
#endif

class DSPMap {
public:
    /* :145-175.  init_particle_num > 0 pre-fills the map with random particles (addRandomParticles
     * :594-624) -- deferred to the first device use so that a global `DSPMap my_map;` is safe. */
    DSPMap(int init_particle_num = 0, float init_weight = 0.01f)
        : init_particles_(init_particle_num), init_weight_(init_weight) {
        dspmap_config cfg;
        dspmap_default_config(&cfg);
        cfg.nx = MAP_LENGTH_VOXEL_NUM; cfg.ny = MAP_WIDTH_VOXEL_NUM; cfg.nz = MAP_HEIGHT_VOXEL_NUM;
        cfg.voxel_resolution = (float)VOXEL_RESOLUTION;
        cfg.angle_resolution = ANGLE_RESOLUTION;
        cfg.max_particle_num_voxel = MAX_PARTICLE_NUM_VOXEL;
        cfg.half_fov_h = half_fov_h; cfg.half_fov_v = half_fov_v;
        cfg.prediction_times = PREDICTION_TIMES;
        for (int i = 0; i < PREDICTION_TIMES; i++) cfg.prediction_future_time[i] = prediction_future_time[i];
        // the reference's two other headers are parameter sets of the same kernels:
        //   dsp_dynamic_multiple_neighbors.h: -DANGLE_RESOLUTION=1 -DPYRAMID_NEIGHBOR_N=2 (+ its map macros, :38-51)
        //   dsp_static.h: -DDSPMAP_STATIC_MODEL=1 -DDSPMAP_SAFE_PARTICLE_FACTOR=5 -DPREDICTION_TIMES=1 (:46-47,63,640-646)
        // both test occlusion with VOXEL_RESOLUTION instead of 0.3 m (:761 there): -DDSPMAP_OCCLUSION_MARGIN=VOXEL_RESOLUTION
#ifdef PYRAMID_NEIGHBOR_N
        cfg.pyramid_neighbor_n = PYRAMID_NEIGHBOR_N;
#endif
#ifdef DSPMAP_SAFE_PARTICLE_FACTOR
        cfg.safe_particle_factor = DSPMAP_SAFE_PARTICLE_FACTOR;
#endif
#ifdef DSPMAP_STATIC_MODEL
        cfg.static_model = DSPMAP_STATIC_MODEL;
#endif
#ifdef DSPMAP_WORLD
        // Z-slab sharding across the GPUs of one node (-DDSPMAP_WORLD): one process per GPU, started by any launcher that
        // exports RANK / WORLD_SIZE / LOCAL_RANK (torchrun, mpirun wrappers).  This rank owns the layers [z_lo, z_hi); every
        // rank is fed the same cloud and pose; update() runs the C++ RCCL frame driver (dspmap_mgpu_update_host).  The
        // getters return this rank's slab (voxel indices stay global).
        {
            const char* wr = getenv("WORLD_SIZE"); const char* rk = getenv("RANK"); const char* lr = getenv("LOCAL_RANK");
            world_ = wr ? atoi(wr) : 1; rank_ = rk ? atoi(rk) : 0;
            if (world_ > 1) {
                const int base = cfg.nz / world_, rem = cfg.nz % world_;
                cfg.z_lo = rank_ * base + (rank_ < rem ? rank_ : rem);
                cfg.z_hi = cfg.z_lo + base + (rank_ < rem ? 1 : 0);
            }
            cfg.device = lr ? atoi(lr) : -1;
        }
#endif
        h_ = dspmap_create(&cfg);
        if (h_) dspmap_set_param(h_, DSPMAP_P_VELOCITY_ESTIMATOR, DSPMAP_ESTIMATOR_MODE);  // update() runs the velocity estimator like :297
#ifdef DSPMAP_OCCLUSION_MARGIN
        if (h_) dspmap_set_param(h_, DSPMAP_P_OCCLUSION_MARGIN, (double)(DSPMAP_OCCLUSION_MARGIN));
#endif
        cout << "Map is ready to update!" << endl;  // :174
    }
    ~DSPMap() {  // :177-179
        dspmap_destroy(h_);
        cout << "\n See you ;)" << endl;
    }
    DSPMap(const DSPMap&) = delete;
    DSPMap& operator=(const DSPMap&) = delete;

    /* :181-353.  Returns 1, or 0 when the frame is rejected (state untouched, :193-208). */
    int update(int point_cloud_num, int size_of_one_point, float* point_cloud_ptr, float sensor_px, float sensor_py,
               float sensor_pz, double time_stamp_second, float sensor_quaternion_w, float sensor_quaternion_x,
               float sensor_quaternion_y, float sensor_quaternion_z) {
        lazy_prefill();
#ifdef DSPMAP_WORLD
        if (!comm_ready_) {   // the communicator is created at the first frame: no HIP / RCCL call during static initialisation
            if (dspmap_mgpu_comm_init_from_env(h_) != DSPMAP_OK) { cerr << "DSPMap: " << dspmap_last_error(h_) << endl; return 0; }
            comm_ready_ = true;
        }
        const int rc = dspmap_mgpu_update_host(h_, point_cloud_num, size_of_one_point, point_cloud_ptr, sensor_px, sensor_py,
                                               sensor_pz, time_stamp_second, sensor_quaternion_w, sensor_quaternion_x,
                                               sensor_quaternion_y, sensor_quaternion_z);
#else
        const int rc = dspmap_update(h_, point_cloud_num, size_of_one_point, point_cloud_ptr, sensor_px, sensor_py,
                                     sensor_pz, time_stamp_second, sensor_quaternion_w, sensor_quaternion_x,
                                     sensor_quaternion_y, sensor_quaternion_z);
#endif
        if (rc < 0) { cerr << "DSPMap::update failed: " << dspmap_last_error(h_) << endl; return 0; }
        record_hook(rc);
        return rc;
    }

    /* No counterpart in the reference: the whole frame from one depth image in host memory (16UC1 / 32FC1, described by `cam`) --
       back-projection, the voxel-grid centroid filter (leaf), axis swap, crop and cap (max_points) run on the device
       (dspmap_update_depth, include/dspmap.h), so the node's cloudCallback pre-processing (src/map_sim_example.cpp:309-336) and its
       point-cloud copy go away.  Returns 1, 0 (rejected) like update(); a negative code on an error (text on cerr).  Sharded
       builds (-DDSPMAP_WORLD) keep the cloud entry point: DSPMAP_E_STATE. */
    int updateDepth(const dspmap_camera& cam, const void* depth_host, float sensor_px, float sensor_py, float sensor_pz,
                    double time_stamp_second, float sensor_quaternion_w, float sensor_quaternion_x, float sensor_quaternion_y,
                    float sensor_quaternion_z, float leaf = 0.1f, int max_points = 5000) {
#ifdef DSPMAP_WORLD
        (void)cam; (void)depth_host; (void)sensor_px; (void)sensor_py; (void)sensor_pz; (void)time_stamp_second;
        (void)sensor_quaternion_w; (void)sensor_quaternion_x; (void)sensor_quaternion_y; (void)sensor_quaternion_z; (void)leaf; (void)max_points;
        return DSPMAP_E_STATE;
#else
        lazy_prefill();
        const float pos[3] = {sensor_px, sensor_py, sensor_pz};
        const float quat[4] = {sensor_quaternion_w, sensor_quaternion_x, sensor_quaternion_y, sensor_quaternion_z};
        const int rc = dspmap_update_depth(h_, &cam, depth_host, leaf, max_points, pos, time_stamp_second, quat);
        if (rc < 0) { cerr << "DSPMap::updateDepth failed: " << dspmap_last_error(h_) << endl; return rc; }
        record_hook(rc);
        return rc;
#endif
    }

    void setPredictionVariance(float p_stddev, float v_stddev) {  // :355-360 (regenerates the Gaussian tables)
        dspmap_set_param(h_, DSPMAP_P_POSITION_STDDEV, p_stddev);
        dspmap_set_param(h_, DSPMAP_P_VELOCITY_STDDEV, v_stddev);
        dspmap_set_param(h_, DSPMAP_P_REGENERATE_TABLES, 1);
    }
    void setObservationStdDev(float ob_stddev) { dspmap_set_param(h_, DSPMAP_P_OBSERVATION_STDDEV, ob_stddev); }  // :362
    void setNewBornParticleWeight(float weight) { dspmap_set_param(h_, DSPMAP_P_NEWBORN_WEIGHT, weight); }        // :366
    void setNewBornParticleNumberofEachPoint(int num) { dspmap_set_param(h_, DSPMAP_P_NEWBORN_NUMBER, num); }      // :370
    /* :375-378.  Arms the particle CSV dump at the end of update() (:326-350); writeParticleCsv() writes one on request. */
    void setParticleRecordFlag(int record_particle_flag, float record_csv_time = 1.f) {
        record_flag_ = record_particle_flag; record_time_ = record_csv_time;
    }
    static void setOriginalVoxelFilterResolution(float res) { voxel_filter_res() = res; }  // :380 (static in the reference)

    void getOccupancyMap(int& obstacles_num, pcl::PointCloud<pcl::PointXYZ>& cloud, const float threshold = 0.7) {  // :385-402
        fetch(obstacles_num, cloud, nullptr, threshold);
    }
    void getOccupancyMapWithFutureStatus(int& obstacles_num, pcl::PointCloud<pcl::PointXYZ>& cloud, float* future_status,
                                         const float threshold = 0.7) {  // :405-426
        fetch(obstacles_num, cloud, future_status, threshold);
    }
    /* north-star name: the V x T future occupancy masses (then cleared, like the getters above) */
    void getFutureStatus(float* future_status) { sync_params(); dspmap_get_future(h_, future_status + (size_t)dspmap_local_voxel_base(h_) * PREDICTION_TIMES); }
    /* extensions: read-only point / trajectory queries on the device (dspmap_query_occupancy / dspmap_trajectory_risk in dspmap.h):
     * values[i] = predicted occupancy around samples[i] = {x, y, z, t} within `radius` (t < 0: current mass, else the first
     * horizon >= t); no whole-grid copy, nothing cleared.  Return DSPMAP_OK or a negative dspmap.h error code. */
    int queryOccupancy(int n, const dspmap_query* samples, float* values, float radius = 0.f, bool world_frame = false,
                       float outside_value = 1.f) {
        return dspmap_query_occupancy(h_, n, samples, radius, world_frame ? DSPMAP_QUERY_WORLD : 0, outside_value, values);
    }
    int evaluateTrajectories(int n_traj, int n_samples, const dspmap_query* samples, dspmap_risk* risk, float radius = 0.f,
                             bool world_frame = false, float outside_value = 1.f, const float threshold = 0.7) {
        return dspmap_trajectory_risk(h_, n_traj, n_samples, samples, radius, world_frame ? DSPMAP_QUERY_WORLD : 0, outside_value,
                                      threshold, risk);
    }
    /* extensions: truncated Euclidean distance fields of the current (layer 0) and the predicted (layer 1 + k) occupancy, built and kept on
     * the device (dspmap_build_distance_field in dspmap.h): metres to the nearest voxel with mass > threshold, at most max_voxels voxels.
     * Read-only towards the map; a field is a snapshot and goes stale with the next update().  Return DSPMAP_OK or a negative error code. */
    int buildDistanceField(const float threshold = 0.7, int max_voxels = 20, bool outside_occupied = false) {
        return dspmap_build_distance_field(h_, threshold, max_voxels, outside_occupied ? DSPMAP_DIST_OUTSIDE_OCCUPIED : 0);
    }
    int getDistanceField(int layer, float* field) { return dspmap_get_distance_field(h_, layer, field); }
    int queryDistance(int n, const dspmap_query* samples, float* distances, float* gradients = nullptr, bool world_frame = false,
                      float outside_value = 0.f) {
        return dspmap_query_distance(h_, n, samples, world_frame ? DSPMAP_QUERY_WORLD : 0, outside_value, distances, gradients);
    }
    /* extensions: nearest-obstacle fields of the same layers (dspmap_build_nearest_field in dspmap.h): per voxel the global index of the
     * nearest occupied voxel within max_voxels voxels (-1: none; ties: the smallest index) and the distance to it.  is_signed: an occupied
     * voxel gets its nearest free voxel and a negative distance; from_cast_grid: occupied is what buildCastGrid() left (threshold unread).
     * queryNearest gives per sample the own voxel's pair, the offset to that voxel's centre and, in the current layer, its velocity.
     * Read-only towards the map; a snapshot like the distance field.  Return DSPMAP_OK or a negative error code. */
    int buildNearestField(const float threshold = 0.7, int max_voxels = 20, bool is_signed = false, bool from_cast_grid = false) {
        return dspmap_build_nearest_field(h_, threshold, max_voxels,
                                          (is_signed ? DSPMAP_NEAREST_SIGNED : 0) | (from_cast_grid ? DSPMAP_NEAREST_FROM_CAST_GRID : 0));
    }
    int getNearestField(int layer, int* nearest, float* distances = nullptr) { return dspmap_get_nearest_field(h_, layer, nearest, distances); }
    int queryNearest(int n, const dspmap_query* samples, dspmap_nearest* out, bool world_frame = false, float outside_value = 0.f) {
        return dspmap_query_nearest(h_, n, samples, world_frame ? DSPMAP_QUERY_WORLD : 0, outside_value, out);
    }
    /* extensions: segment casts through bit grids of the current (layer 0) and the predicted (layer 1 + k) occupancy, built and kept on the
     * device (dspmap_build_cast_grid in dspmap.h): hits[i] = the first cell of segs[i] = {a, ta, b, tb} whose bit is set, tested in the
     * horizon of the time the segment enters it.  Read-only towards the map; a grid is a snapshot and goes stale with the next update().
     * Return DSPMAP_OK or a negative error code. */
    int buildCastGrid(float thr = 0.2f, int inflate = 0) { return dspmap_build_cast_grid(h_, thr, inflate, 0); }
    int castSegments(int n, const dspmap_segment* segs, dspmap_cast_hit* hits, bool world = false) {
        return dspmap_cast_segments(h_, n, segs, world ? DSPMAP_QUERY_WORLD : 0, hits);
    }
    /* extension: axis-aligned free boxes (safe corridors) grown in the cast grid around the pieces seeds[i] = {a, ta, b, tb} of a path
     * (dspmap_grow_boxes in dspmap.h): boxes[i] = inclusive voxel bounds, a status and the cause that stopped each face.  Needs a grid
     * built by buildCastGrid() since the last update(); read-only.  Return DSPMAP_OK or a negative error code. */
    int growBoxes(int n, const dspmap_segment* seeds, const int max_grow[3], dspmap_box* boxes, bool world = false, bool with_current = false) {
        return dspmap_grow_boxes(h_, n, seeds, max_grow, (world ? DSPMAP_QUERY_WORLD : 0) | (with_current ? DSPMAP_BOX_WITH_CURRENT : 0), boxes);
    }
    /* extension: arrival-time fields grown through the cast grid (dspmap_build_reach_fields in dspmap.h): n_fields fields, each from the
     * sources src[i] = {x, y, z, field} that name it; step n happens at t_start + n * step_seconds and tests the layer of that time
     * (t_start < 0: the current layer).  Needs a grid built by buildCastGrid() since the last update(); read-only.  getReachField copies
     * one field's V uint16 values (DSPMAP_REACH_UNREACHED where the front never came); reachPaths descends a time-invariant build from
     * starts[i] (steps[i] = the start's value or a negative cause, cells[i * max_len + j] = voxel indices, -1 behind the path's end).
     * Return DSPMAP_OK or a negative error code. */
    int buildReachFields(int n_fields, int n_src, const dspmap_reach_point* src, float t_start, float step_seconds, int max_steps,
                         bool world = false, bool with_current = false) {
        return dspmap_build_reach_fields(h_, n_fields, n_src, src, t_start, step_seconds, max_steps,
                                         (world ? DSPMAP_QUERY_WORLD : 0) | (with_current ? DSPMAP_REACH_WITH_CURRENT : 0));
    }
    int getReachField(int field, unsigned short* values) { return dspmap_get_reach_field(h_, field, values); }
    int reachPaths(int n, const dspmap_reach_point* starts, int max_len, int* steps, int* cells, bool world = false) {
        return dspmap_reach_paths(h_, n, starts, max_len, world ? DSPMAP_QUERY_WORLD : 0, steps, cells);
    }
    /* extension: space-time paths (dspmap_build_reach_timeline in dspmap.h): buildReachTimeline grows the same fields as buildReachFields and
     * keeps every step's reached set, getReachSets copies n_steps of them (nz * ny * W words each, the cast grid's layer layout) and
     * reachTimelinePaths walks backwards through them -- also where the tested layer changed during the steps, which reachPaths refuses:
     * cells[i * max_len + j] = the voxel occupied at step steps[i] - j, waits included.  Return DSPMAP_OK or a negative error code. */
    int buildReachTimeline(int n_fields, int n_src, const dspmap_reach_point* src, float t_start, float step_seconds, int max_steps,
                           bool world = false, bool with_current = false) {
        return dspmap_build_reach_timeline(h_, n_fields, n_src, src, t_start, step_seconds, max_steps,
                                           (world ? DSPMAP_QUERY_WORLD : 0) | (with_current ? DSPMAP_REACH_WITH_CURRENT : 0));
    }
    int getReachSets(int field, int first_step, int n_steps, unsigned long long* words) {
        return dspmap_get_reach_sets(h_, field, first_step, n_steps, words);
    }
    int reachTimelinePaths(int n, const dspmap_reach_point* starts, int max_len, int* steps, int* cells, bool world = false) {
        return dspmap_reach_timeline_paths(h_, n, starts, max_len, world ? DSPMAP_QUERY_WORLD : 0, steps, cells);
    }
    /* extension: paths cut down to line-of-sight waypoints (dspmap_shorten_paths in dspmap.h): steps and cells as reachPaths and
     * reachTimelinePaths write them (or any polyline of voxel indices ended by -1); from each anchor the farthest of the next `window`
     * cells that castSegments calls free.  With the build's t_start and step_seconds every cell keeps the time of its step.  info[i] =
     * {n_cells, n_segments, n_blocked, truncated}, segs[i * max_seg + s] = records castSegments and growBoxes take, ends[i * max_seg + s] =
     * the path position segment s ends at.  Needs a grid built by buildCastGrid() since the last update(); read-only.  Return DSPMAP_OK or
     * a negative error code. */
    int shortenPaths(int n, int max_len, const int* steps, const int* cells, float t_start, float step_seconds, int window, int max_seg,
                     dspmap_path_info* info, dspmap_segment* segs, int* ends) {
        return dspmap_shorten_paths(h_, n, max_len, steps, cells, t_start, step_seconds, window, max_seg, 0, info, segs, ends);
    }
    /* extension: clearance-weighted cost-to-go fields (dspmap_build_cost_fields in dspmap.h): the wavefront of buildReachFields through ONE
     * layer (t < 0: the current one), the step into a free cell costing 1 plus the penalty of every band whose clearance the cell's value
     * in the distance field lies under.  Needs buildCastGrid() and, with bands, buildDistanceField() since the last update(); read-only.
     * getCostField copies one field's V uint16 values (DSPMAP_COST_UNREACHED above max_cost), getCostWeights the V weight bytes (0 blocked);
     * costPaths descends from starts[i] (cost[i] = the start's value or a negative cause, cells as reachPaths) -- what shortenPaths takes.
     * Return DSPMAP_OK or a negative error code. */
    int buildCostFields(int n_fields, int n_src, const dspmap_reach_point* src, float t, const dspmap_cost_bands& bands, int max_cost,
                        bool world = false) {
        return dspmap_build_cost_fields(h_, n_fields, n_src, src, t, &bands, max_cost, world ? DSPMAP_QUERY_WORLD : 0);
    }
    int getCostField(int field, unsigned short* values) { return dspmap_get_cost_field(h_, field, values); }
    int getCostWeights(unsigned char* weights) { return dspmap_get_cost_weights(h_, weights); }
    int costPaths(int n, const dspmap_reach_point* starts, int max_len, int* cost, int* cells, bool world = false) {
        return dspmap_cost_paths(h_, n, starts, max_len, world ? DSPMAP_QUERY_WORLD : 0, cost, cells);
    }
    /* extension: occupancy forecast at times of the caller's choosing (dspmap_build_forecast in dspmap.h): layer j = the mass of every live
     * particle, newborns included, rolled out to times[j] seconds after the last update() -- strictly ascending, at most
     * DSPMAP_FORECAST_MAX_TIMES.  Read-only towards the map; a snapshot that goes stale with the next update().  getForecast copies one
     * layer's V floats; queryForecast reads each sample's own voxel in the first layer at or after its t, or with lerp interpolates between
     * that layer and the one before.  Return DSPMAP_OK or a negative error code. */
    int buildForecast(int n_times, const float* times) { return dspmap_build_forecast(h_, n_times, times, 0); }
    int getForecast(int layer, float* values) { return dspmap_get_forecast(h_, layer, values); }
    int queryForecast(int n, const dspmap_query* q, float* out, bool world = false, bool lerp = false, float outside_value = 1.f) {
        return dspmap_query_forecast(h_, n, q, (world ? DSPMAP_QUERY_WORLD : 0) | (lerp ? DSPMAP_FORECAST_LERP : 0), outside_value, out);
    }
    /* extension: known space (dspmap_known_integrate in dspmap.h): remember which voxels the last update()'s view reached -- inside a
     * pyramid, not behind its farthest return, within max_range -- anchored in the world, so that "free because observed" stays apart
     * from "free because nobody looked".  getKnownAge copies V ages (frames since a voxel was last seen, -1 = never), queryKnown reads
     * the age at sample points, maskCastGridUnknown marks every voxel older than max_age (or never seen) as blocked in all layers of the
     * cast grid, for the casts, boxes and arrival fields that read it.  Return DSPMAP_OK or a negative error code. */
    int integrateKnownSpace(float max_range = INFINITY) { return dspmap_known_integrate(h_, max_range, 0); }
    int getKnownAge(int* ages) { return dspmap_get_known(h_, ages); }
    int queryKnown(int n, const dspmap_query* q, int* ages, bool world = false) {
        return dspmap_query_known(h_, n, q, world ? DSPMAP_QUERY_WORLD : 0, ages);
    }
    int maskCastGridUnknown(int max_age) { return dspmap_mask_cast_grid(h_, max_age, 0); }
    /* extension: scores of candidate viewpoints (dspmap_score_views in dspmap.h): for every view {position, attitude, max_range, t} the
     * voxels a frame taken from there would see through the cast grid as it is (n_seen), those of them that are unknown now -- never
     * seen, or seen more than max_age frames ago -- (n_unknown), and the rays that ended on an obstacle (n_returns).  viewRays hands out
     * the rotated planes and ray directions of an attitude (any pointer may be NULL).  Return DSPMAP_OK or a negative error code. */
    int scoreViews(int n, const dspmap_view* views, int max_age, dspmap_view_score* scores, bool world = false) {
        return dspmap_score_views(h_, n, views, max_age, world ? DSPMAP_QUERY_WORLD : 0, scores);
    }
    int viewRays(const float quat_wxyz[4], float* planes_h, float* planes_v, float* dirs) {
        return dspmap_view_rays(h_, quat_wxyz, planes_h, planes_v, dirs);
    }
    /* extension: joint gain of views (dspmap_score_view_sets in dspmap.h): scoreViewSets gives, for every set of set_size views
     * (views [n_sets][set_size]; pad a short set with views of max_range 0), the voxels its members see TOGETHER (n_seen), those of them
     * that are unknown now (n_unknown) and its usable members (n_ok).  selectViews picks greedily k of the n views: views [0, n_fixed)
     * are committed already, every round takes the candidate that adds the most unknown voxels to what is covered, until a round's best
     * adds fewer than min_gain (picks[r].view = -1 from there on).  view_scores (may be NULL) receives what scoreViews gives per view.
     * Return DSPMAP_OK or a negative error code. */
    int scoreViewSets(int n_sets, int set_size, const dspmap_view* views, int max_age, dspmap_view_set_score* set_scores,
                      dspmap_view_score* view_scores = nullptr, bool world = false) {
        return dspmap_score_view_sets(h_, n_sets, set_size, views, max_age, world ? DSPMAP_QUERY_WORLD : 0, set_scores, view_scores);
    }
    int selectViews(int n, const dspmap_view* views, int k, int max_age, dspmap_view_pick* picks, int n_fixed = 0, int min_gain = 1,
                    dspmap_view_score* view_scores = nullptr, bool world = false) {
        return dspmap_select_views(h_, n, views, n_fixed, max_age, world ? DSPMAP_QUERY_WORLD : 0, k, min_gain, picks, view_scores);
    }
    /* extension: frontiers (dspmap_build_frontiers in dspmap.h): the known cells (0 <= age <= max_age) with a clear bit in the layer t
     * selects of the cast grid and at least min_unknown unknown face neighbours, as an ascending list of voxel indices and summed over
     * blocks of block^3 voxels, whose centroids (sum / count) are where a planner puts its candidate views.  buildFrontiers enqueues;
     * the getters copy the first min(cap, n) entries and report n.  Return DSPMAP_OK or a negative error code. */
    int buildFrontiers(int max_age, int min_unknown = 1, int block = 4, float t = -1.f) {
        return dspmap_build_frontiers(h_, t, max_age, min_unknown, block, 0);
    }
    int getFrontierCells(int cap, int* cells, int& n) { return dspmap_get_frontier_cells(h_, cap, cells, &n); }
    int getFrontierBlocks(int cap, dspmap_frontier_block* blocks, int& n) { return dspmap_get_frontier_blocks(h_, cap, blocks, &n); }
    /* extension: objects (dspmap_build_objects in dspmap.h): the connected components (connectivity 6 or 26) of the layer t selects of
     * the cast grid, those with at least min_cells cells as records -- box, index sums (centroid = sum / count), fixed-point mass and
     * momentum of the current result grid (velocity = mom_q / mass_q) -- in ascending label, at most max_objects of them.  buildObjects
     * enqueues; getObjects copies the first min(cap, n) records and reports n; queryObjects gives, per sample {x, y, z, t} (t ignored),
     * the ordinal of the object that holds it or -1.  Return DSPMAP_OK or a negative error code. */
    int buildObjects(int connectivity = 26, int min_cells = 1, int max_objects = 4096, float t = -1.f) {
        return dspmap_build_objects(h_, t, connectivity, min_cells, max_objects, 0);
    }
    int getObjects(int cap, dspmap_object* objects, int& n) { return dspmap_get_objects(h_, cap, objects, &n); }
    int queryObjects(int n, const dspmap_query* samples, int* ordinals, bool world = false) {
        return dspmap_query_objects(h_, n, samples, world ? DSPMAP_QUERY_WORLD : 0, ordinals);
    }
    /* extension: tracks (dspmap_track_update in dspmap.h): after buildObjects, trackObjects associates the objects with those of the
     * previous call by voxel overlap -- predicted by each object's velocity over dt seconds, at most max_shift voxels -- and gives every
     * record a dspmap_track with the same index: an id that persists while the object is matched, its age, the id it split off from.
     * trackObjects enqueues; getTracks copies the first min(cap, n) tracks and reports n; resetTracks forgets everything and starts the
     * ids at 0 again.  Return DSPMAP_OK or a negative error code. */
    int trackObjects(float dt, int min_overlap = 1, int max_shift = 8, int max_pairs = 0) {
        return dspmap_track_update(h_, dt, min_overlap, max_shift, max_pairs, 0);
    }
    int getTracks(int cap, dspmap_track* tracks, int& n) { return dspmap_get_tracks(h_, cap, tracks, &n); }
    int resetTracks() { return dspmap_track_reset(h_); }
    void clearOccupancyMapPrediction() { dspmap_clear_future(h_); }  // :431-438

    void getKMClusterResult(pcl::PointCloud<pcl::PointXYZINormal>& cluster_cloud) {  // :441-445
        int n = 0;
        dspmap_get_birth_cloud(h_, nullptr, 0, &n);
        std::vector<dspmap_vpoint> v((size_t)n);
        if (n) dspmap_get_birth_cloud(h_, v.data(), n, &n);
        for (const auto& q : v) {
            pcl::PointXYZINormal p;
            p.x = q.x; p.y = q.y; p.z = q.z;
            p.normal_x = q.nx; p.normal_y = q.ny; p.normal_z = q.nz; p.intensity = q.intensity;
            cluster_cloud.push_back(p);
        }
    }

    void mapAddNewBornParticlesByObservation() { dspmap_stage_birth(h_); }  // public in the reference (:796)

    static float generateRandomFloat(float min, float max) {  // :1551-1553
        return min + static_cast<float>(rand()) / (static_cast<float>(RAND_MAX / (max - min)));
    }
    void getVoxelPositionFromIndexPublic(const int& index, float& px, float& py, float& pz) const {  // :1556-1572
        dspmap_voxel_center(h_, index, &px, &py, &pz);
    }
    int getPointVoxelsIndexPublic(const float& px, const float& py, const float& pz, int& index) {  // :1574-1584
        return dspmap_point_voxel_index(h_, px, py, pz, &index);
    }

    /* particle CSV in the reference's column order (:336-347): flag,vx,vy,vz,px,py,pz,weight,voxel_index */
    int writeParticleCsv(const std::string& file_name) {
        int n = 0;
        dspmap_export_state(h_, 0, nullptr, nullptr, nullptr, &n);
        std::vector<int> vox((size_t)n), slot((size_t)n);
        std::vector<float> rec((size_t)n * 8);
        if (n) dspmap_export_state(h_, n, vox.data(), slot.data(), rec.data(), &n);
        // the reference walks voxels, then slots, in ascending order (:337-338); the device compaction is unordered
        std::vector<int> order((size_t)n);
        for (int i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return vox[a] != vox[b] ? vox[a] < vox[b] : slot[a] < slot[b]; });
        std::ofstream w(file_name, std::ios::out | std::ios::trunc);
        for (int q = 0; q < n; q++) {
            const int i = order[q];
            for (int k = 0; k < 8; k++) w << rec[(size_t)i * 8 + k] << ",";
            w << vox[i] << "\n";
        }
        return n;
    }

    dspmap_t* dspmap_handle() { return h_; }

private:
    static float& voxel_filter_res() { static float r = 0.15f; return r; }  // :132
    void sync_params() { dspmap_set_param(h_, DSPMAP_P_VOXEL_FILTER_RES, voxel_filter_res()); }
    void record_hook(int rc) {   // :326-350: every frame when the flag is negative, else once after record_time
        if (rc != 1 || !record_flag_) return;
        const float update_time = (float)dspmap_get_param(h_, DSPMAP_P_UPDATE_TIME);
        if (record_flag_ < 0 || (update_time > record_time_ && !recorded_once_)) {
            recorded_once_ = 1;
            const int update_counter = (int)dspmap_get_param(h_, DSPMAP_P_UPDATE_COUNTER);
            writeParticleCsv(particle_save_folder + "/particles_update_t_" + to_string(update_counter) + "_" +
                             to_string((int)(update_time * 1000)) + ".csv");
        }
    }
    void lazy_prefill() {
        sync_params();
        if (init_particles_ > 0) { dspmap_add_random_particles(h_, init_particles_, init_weight_); init_particles_ = 0; }
    }
    void fetch(int& obstacles_num, pcl::PointCloud<pcl::PointXYZ>& cloud, float* future_status, float threshold) {
        const int v = dspmap_local_voxel_num(h_);
        xyz_.resize((size_t)v * 3);
        int n = 0;
        // a slab's rows land at their GLOBAL voxel offsets of the caller's [VOXEL_NUM][PREDICTION_TIMES] array
        if (future_status) future_status += (size_t)dspmap_local_voxel_base(h_) * PREDICTION_TIMES;
        const int rc = future_status ? dspmap_get_occupancy_with_future(h_, threshold, xyz_.data(), v, &n, future_status)
                                     : dspmap_get_occupancy(h_, threshold, xyz_.data(), v, &n);
        obstacles_num = rc == DSPMAP_OK ? n : 0;
        for (int i = 0; i < obstacles_num; i++) {  // appended, never cleared by the map (:391,411)
            pcl::PointXYZ p;
            p.x = xyz_[3 * (size_t)i]; p.y = xyz_[3 * (size_t)i + 1]; p.z = xyz_[3 * (size_t)i + 2];
            cloud.push_back(p);
        }
    }
    dspmap_t* h_ = nullptr;
#ifdef DSPMAP_WORLD
    int world_ = 1, rank_ = 0;
    bool comm_ready_ = false;
#endif
    int init_particles_;
    float init_weight_;
    int record_flag_ = 0;        // if_record_particle_csv :479
    float record_time_ = 1.f;    // record_time :480
    int recorded_once_ = 0;      // recorded_once_flag :326
    std::vector<float> xyz_;
};

#endif /* DSP_DYNAMIC_H_MI355X */
