// dspmap_layers.hip -- host side of the planning layers that read the map: point and trajectory queries, distance fields, the cast grid with
// segment casts and free boxes, arrival-time fields with timeline and paths, shortened paths, cost-to-go fields, the forecast, the known-space layer, view scores, view sets and selection, and frontiers.
// Their kernels are in a file each (named per section); their state is LayerState (dspmap_internal.h), and what makes a snapshot stale is
// decided in ONE place, dspmap_layers_stale next to it.  An entry point that takes host arrays is: check -> stage -> enqueue -> read back,
// around the same *_enqueue its _device twin calls.  Checks fire in this order: arguments, slab and state, then the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "dspmap_grid.h"   // SampleOrigin's users, grid_layer_words
#include "dspmap_internal.h"

// --------------------------------------------------- checks and argument fills every layer repeats
// these layers need the whole map: `why` is the layer's own sentence (may be empty)
static int whole_map_check(dspmap* m, const char* what, const char* why) {
    if (m->d.z_lo != 0 || m->d.z_hi != m->d.nz)
        return dspmap_fail(m, DSPMAP_E_STATE, "%s: a slab handle holds part of the map%s%s", what, *why ? "; " : "", why);
    return DSPMAP_OK;
}
// n items (`noun`) in one array, as many results in another
static int samples_check(dspmap* m, const char* what, const char* noun, long long n, const void* in, const void* out) {
    if (n < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative %s count %lld", what, noun, n);
    if (n > 0 && (!in || !out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL %s or output array", what, noun);
    return DSPMAP_OK;
}
static int flags_check(dspmap* m, const char* what, int flags, int allowed) {
    if (flags & ~allowed) return dspmap_fail(m, DSPMAP_E_ARG, "%s: unknown flags 0x%x", what, flags);
    return DSPMAP_OK;
}
// a snapshot's readers: stale or never built is a state error with the layer's sentence `missing`; the handle's device is made current
// (these entry points queue work without going through READY)
static int snapshot_ready(dspmap* m, bool valid, const char* what, const char* missing) {
    if (!valid) return dspmap_fail(m, DSPMAP_E_STATE, "%s: %s", what, missing);
    if (m->device >= 0) (void)hipSetDevice(m->device);
    return DSPMAP_OK;
}
// the origin of the samples' coordinates: the sensor position of the last update when DSPMAP_QUERY_WORLD is set
static SampleOrigin origin_fill(const dspmap* m, int flags) {
    return SampleOrigin{m->cur_pos[0], m->cur_pos[1], m->cur_pos[2], (flags & DSPMAP_QUERY_WORLD) ? 1 : 0};
}
// a layer's scratch buffer of at least `need` items; the caller has drained the stream (an earlier call may still read the old one)
template <class T> static int layer_buf_grow(dspmap* m, T** p, size_t* have, size_t need) {
    if (need <= *have) return DSPMAP_OK;
    if (*p) { HIPCHK(m, hipFree(*p)); *p = nullptr; *have = 0; }
    HIPCHK(m, hipMalloc(p, sizeof(T) * need));
    *have = need;
    return DSPMAP_OK;
}

// --------------------------------------------------- staging of the host variants' arrays (LayerState::q_buf)
static size_t q_align(size_t b) { return (b + 255) & ~(size_t)255; }
// the handle's query staging: at least `bytes`; grown only after the stream has drained (an earlier query may still use it)
static int query_buf(dspmap* m, size_t bytes) {
    if (bytes <= m->ly.q_buf_bytes) return DSPMAP_OK;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (m->ly.q_buf) { HIPCHK(m, hipFree(m->ly.q_buf)); m->ly.q_buf = nullptr; m->ly.q_buf_bytes = 0; }
    const size_t cap = bytes + bytes / 2;
    HIPCHK(m, hipMalloc(&m->ly.q_buf, cap));
    m->ly.q_buf_bytes = cap;
    return DSPMAP_OK;
}
// one section of the staging buffer, 256-byte aligned: `in` is copied into it before the launches, it is copied to `out` behind them; either
// may be NULL (scratch, or an output the caller did not ask for).  dev: where it lies, NULL for a section of no bytes
struct StageSec { const void* in; void* out; size_t bytes; void* dev; };
// reserves the sections in their order, grows the buffer and queues the copies in
static int stage_begin(dspmap* m, StageSec* s, int n_sec) {
    size_t end = 0;
    for (int i = 0; i < n_sec; ++i) if (s[i].bytes) end = q_align(end) + s[i].bytes;
    const int rc = query_buf(m, end);
    if (rc != DSPMAP_OK) return rc;
    end = 0;
    for (int i = 0; i < n_sec; ++i) {
        s[i].dev = nullptr;
        if (!s[i].bytes) continue;
        s[i].dev = (char*)m->ly.q_buf + q_align(end);
        end = q_align(end) + s[i].bytes;
        if (s[i].in) HIPCHK(m, hipMemcpyAsync(s[i].dev, s[i].in, s[i].bytes, hipMemcpyHostToDevice, m->stream));
    }
    return DSPMAP_OK;
}
// a result the device already holds: copied out, and the stream waited for
static int read_back(dspmap* m, void* out, const void* dev, size_t bytes) {
    HIPCHK(m, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return DSPMAP_OK;
}
// queues the copies out in the sections' order and waits for the stream
static int stage_end(dspmap* m, const StageSec* s, int n_sec) {
    for (int i = 0; i < n_sec; ++i)
        if (s[i].bytes && s[i].out) HIPCHK(m, hipMemcpyAsync(s[i].out, s[i].dev, s[i].bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return DSPMAP_OK;
}

// --------------------------------------------------- point / trajectory queries (dspmap_query.hip; semantics in include/dspmap.h)
// argument checks of every query entry point: before READY, so that they hold without a device
static int query_check(dspmap* m, long long n, const void* in, const void* out, float r, int flags, float outside) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if (!(r >= 0.f && r <= 8.f * m->d.res)) return dspmap_fail(m, DSPMAP_E_ARG, "query: radius %g outside [0, 8 * voxel_resolution]", (double)r);
    if ((rc = flags_check(m, "query", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    if (outside != outside) return dspmap_fail(m, DSPMAP_E_ARG, "query: outside_value is NaN");
    return DSPMAP_OK;
}
static QueryArgs query_args(const dspmap* m, float r, int flags, float outside) {
    const MapDims& d = m->d;
    QueryArgs a;
    a.org = origin_fill(m, flags);
    a.r2 = r * r;
    a.K = r > 0.f ? (int)ceilf(r / d.res) + 1 : 0;   // (a superset of the footprint: one lattice step of margin for the rounding)
    a.outside = outside;
    a.fut_zero = m->fut_clear_pending ? 1 : 0;       // read, never changed: the clear stays with the next frame / reader
    a.cx = -d.half_x + d.res * 0.5f; a.cy = -d.half_y + d.res * 0.5f; a.cz = -d.half_z + d.res * 0.5f;   // dspmap_voxel_center
    return a;
}
static int risk_check(dspmap* m, int n_traj, int n_samples, const void* in, const void* out, float r, int flags, float outside) {
    if (!m) return DSPMAP_E_ARG;
    if (n_traj < 0) return dspmap_fail(m, DSPMAP_E_ARG, "trajectory risk: negative trajectory count %d", n_traj);
    if (n_traj > 0 && n_samples <= 0) return dspmap_fail(m, DSPMAP_E_ARG, "trajectory risk: %d samples per trajectory", n_samples);
    const long long n = (long long)n_traj * (n_traj > 0 ? n_samples : 0);
    if (n > 0x7fffffffll) return dspmap_fail(m, DSPMAP_E_ARG, "trajectory risk: %d x %d samples exceed INT_MAX", n_traj, n_samples);
    const int rc = query_check(m, n, in, out, r, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    return whole_map_check(m, "trajectory risk", "query every slab and merge with max");
}

static int query_enqueue(dspmap* m, int n, const float4* dq, float r, int flags, float outside, float* dout) {
    launch_query(dspmap_ctx_of(m), query_args(m, r, flags, outside), n, dq, dout, nullptr);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_occupancy(dspmap_t* m, int n, const dspmap_query* q, float r, int flags, float outside, float* out) {
    int rc = query_check(m, n, q, out, r, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, out, sizeof(float) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = query_enqueue(m, n, (const float4*)s[0].dev, r, flags, outside, (float*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_query_occupancy_device(dspmap_t* m, int n, const dspmap_query* q, float r, int flags, float outside, float* out) {
    const int rc = query_check(m, n, q, out, r, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    return query_enqueue(m, n, (const float4*)q, r, flags, outside, out);
}
// values + flags of the n_traj x n_samples samples in the staging buffer at `vals`, then one dspmap_risk per trajectory into `out`
static int risk_enqueue(dspmap* m, int n_traj, int n_samples, const float4* dq, float* vals, float r, int flags, float outside,
                        float thr, dspmap_risk* out) {
    const int n = n_traj * n_samples;
    const LaunchCtx c = dspmap_ctx_of(m);
    unsigned char* fl = (unsigned char*)((char*)vals + q_align(sizeof(float) * (size_t)n));
    launch_query(c, query_args(m, r, flags, outside), n, dq, vals, fl);
    launch_risk_reduce(c, n_traj, n_samples, vals, fl, thr, out);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
static size_t risk_scratch_bytes(long long n) { return q_align(sizeof(float) * (size_t)n) + q_align((size_t)n); }
extern "C" int dspmap_trajectory_risk(dspmap_t* m, int n_traj, int n_samples, const dspmap_query* q, float r, int flags, float outside,
                                      float thr, dspmap_risk* out) {
    int rc = risk_check(m, n_traj, n_samples, q, out, r, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (n_traj == 0) return DSPMAP_OK;
    const int n = n_traj * n_samples;
    StageSec s[3] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, nullptr, risk_scratch_bytes(n)},
                     {nullptr, out, sizeof(dspmap_risk) * (size_t)n_traj}};
    if ((rc = stage_begin(m, s, 3)) != DSPMAP_OK) return rc;
    if ((rc = risk_enqueue(m, n_traj, n_samples, (const float4*)s[0].dev, (float*)s[1].dev, r, flags, outside, thr, (dspmap_risk*)s[2].dev)) != DSPMAP_OK)
        return rc;
    return stage_end(m, s, 3);
}
extern "C" int dspmap_trajectory_risk_device(dspmap_t* m, int n_traj, int n_samples, const dspmap_query* q, float r, int flags,
                                             float outside, float thr, dspmap_risk* out) {
    int rc = risk_check(m, n_traj, n_samples, q, out, r, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (n_traj == 0) return DSPMAP_OK;
    const int n = n_traj * n_samples;
    if ((rc = query_buf(m, risk_scratch_bytes(n))) != DSPMAP_OK) return rc;
    return risk_enqueue(m, n_traj, n_samples, (const float4*)q, (float*)m->ly.q_buf, r, flags, outside, thr, out);
}

// --------------------------------------------------- distance fields (dspmap_distance.hip; semantics in include/dspmap.h)
extern "C" int dspmap_build_distance_field(dspmap_t* m, float thr, int max_voxels, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (thr != thr) return dspmap_fail(m, DSPMAP_E_ARG, "distance field: threshold is NaN");
    if (max_voxels < 1 || max_voxels > 64) return dspmap_fail(m, DSPMAP_E_ARG, "distance field: max_voxels %d outside [1, 64]", max_voxels);
    if (flags & ~DSPMAP_DIST_OUTSIDE_OCCUPIED) return dspmap_fail(m, DSPMAP_E_ARG, "distance field: unknown flags 0x%x", flags);
    const int rc = whole_map_check(m, "distance field", "distances cross slabs");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    const MapDims& d = m->d;
    const size_t cells = (size_t)(d.T + 1) * d.v_glob;
    dspmap_layers_stale(m->ly, LAYERS_DISTANCE_REBUILD);
    if (!m->ly.df_field) {
        HIPCHK(m, hipMalloc(&m->ly.df_field, sizeof(float) * cells));
        HIPCHK(m, hipMalloc(&m->ly.df_g8, cells));
        HIPCHK(m, hipMalloc(&m->ly.df_h16, sizeof(unsigned short) * cells));
    }
    DistArgs a;
    a.thr = thr; a.R = max_voxels; a.outside_occ = (flags & DSPMAP_DIST_OUTSIDE_OCCUPIED) ? 1 : 0;
    a.fut_zero = m->fut_clear_pending ? 1 : 0;   // read, never changed (as the queries)
    a.L = d.T + 1;
    a.g8 = m->ly.df_g8; a.h16 = m->ly.df_h16; a.field = m->ly.df_field;
    launch_distance_field(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    m->ly.df_valid = true;
    return DSPMAP_OK;
}
extern "C" const float* dspmap_distance_field_device(dspmap_t* m) { return (m && m->ly.df_valid) ? m->ly.df_field : nullptr; }
static int dist_field_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.df_valid, what, "no distance field, or the map has changed since it was built (dspmap_build_distance_field)");
}
extern "C" int dspmap_get_distance_field(dspmap_t* m, int layer, float* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "distance field: NULL output array");
    if (layer < 0 || layer > m->d.T) return dspmap_fail(m, DSPMAP_E_ARG, "distance field: layer %d outside [0, %d)", layer, m->d.T + 1);
    const int rc = dist_field_ready(m, "dspmap_get_distance_field");
    if (rc != DSPMAP_OK) return rc;
    const size_t V = (size_t)m->d.v_glob;
    return read_back(m, out, m->ly.df_field + V * layer, sizeof(float) * V);
}
static int dist_query_check(dspmap* m, int n, const void* in, const void* out, int flags, float outside) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "distance query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "distance query", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    if (outside != outside) return dspmap_fail(m, DSPMAP_E_ARG, "distance query: outside_value is NaN");
    return dist_field_ready(m, "dspmap_query_distance");
}
static DistQueryArgs dist_query_args(const dspmap* m, int flags, float outside) {
    DistQueryArgs a;
    a.org = origin_fill(m, flags);
    a.outside = outside;
    a.field = m->ly.df_field;
    return a;
}
static int dist_query_enqueue(dspmap* m, int n, const float4* dq, int flags, float outside, float* dd, float* dg) {
    launch_distance_query(dspmap_ctx_of(m), dist_query_args(m, flags, outside), n, dq, dd, dg);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_distance(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, float* dist, float* grad) {
    int rc = dist_query_check(m, n, q, dist, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[3] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, dist, sizeof(float) * (size_t)n},
                     {nullptr, grad, grad ? sizeof(float) * 3 * (size_t)n : 0}};   // (no grad: no section, the kernel gets NULL)
    if ((rc = stage_begin(m, s, 3)) != DSPMAP_OK) return rc;
    if ((rc = dist_query_enqueue(m, n, (const float4*)s[0].dev, flags, outside, (float*)s[1].dev, (float*)s[2].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 3);
}
extern "C" int dspmap_query_distance_device(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, float* dist, float* grad) {
    const int rc = dist_query_check(m, n, q, dist, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    return dist_query_enqueue(m, n, (const float4*)q, flags, outside, dist, grad);
}

// --------------------------------------------------- nearest-obstacle fields (dspmap_nearest.hip; semantics in include/dspmap.h)
static_assert(sizeof(dspmap_nearest) == 32, "dspmap_nearest is 32 bytes");
static int cast_grid_ready(dspmap* m, const char* what);
extern "C" int dspmap_build_nearest_field(dspmap_t* m, float thr, int max_voxels, int flags) {
    const char* what = "dspmap_build_nearest_field";
    if (!m) return DSPMAP_E_ARG;
    const bool from_grid = (flags & DSPMAP_NEAREST_FROM_CAST_GRID) != 0, sgn = (flags & DSPMAP_NEAREST_SIGNED) != 0;
    if (!from_grid && thr != thr) return dspmap_fail(m, DSPMAP_E_ARG, "%s: threshold is NaN", what);
    if (max_voxels < 1 || max_voxels > 64) return dspmap_fail(m, DSPMAP_E_ARG, "%s: max_voxels %d outside [1, 64]", what, max_voxels);
    int rc = flags_check(m, what, flags, DSPMAP_NEAREST_SIGNED | DSPMAP_NEAREST_FROM_CAST_GRID);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = whole_map_check(m, what, "distances cross slabs")) != DSPMAP_OK) return rc;
    if (from_grid && (rc = cast_grid_ready(m, what)) != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    const MapDims& d = m->d;
    const int L = d.T + 1;
    const size_t cells = (size_t)L * d.v_glob, scratch = cells * (sgn ? 2 : 1);
    dspmap_layers_stale(m->ly, LAYERS_NEAREST_REBUILD);
    if (!m->ly.nr_near) {
        HIPCHK(m, hipMalloc(&m->ly.nr_near, sizeof(int) * cells));
        HIPCHK(m, hipMalloc(&m->ly.nr_dist, sizeof(float) * cells));
    }
    if (scratch > m->ly.nr_x8_cells || scratch > m->ly.nr_key32_cells) {   // grown only after the stream has drained (an earlier build may still use them)
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if ((rc = layer_buf_grow(m, &m->ly.nr_x8, &m->ly.nr_x8_cells, scratch)) != DSPMAP_OK) return rc;
        if ((rc = layer_buf_grow(m, &m->ly.nr_key32, &m->ly.nr_key32_cells, scratch)) != DSPMAP_OK) return rc;
    }
    NearArgs a;
    a.thr = thr; a.R = max_voxels; a.sgn = sgn ? 1 : 0;
    a.fut_zero = m->fut_clear_pending ? 1 : 0;   // read, never changed (as the queries)
    a.L = L;
    a.grid = from_grid ? m->ly.cg_bits : nullptr;
    a.x8 = m->ly.nr_x8; a.key32 = m->ly.nr_key32; a.near = m->ly.nr_near; a.dist = m->ly.nr_dist;
    launch_nearest_field(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    m->ly.nr_from_grid = from_grid;
    m->ly.nr_valid = true;
    return DSPMAP_OK;
}
extern "C" const int* dspmap_nearest_field_device(dspmap_t* m) { return (m && m->ly.nr_valid) ? m->ly.nr_near : nullptr; }
extern "C" const float* dspmap_nearest_distance_device(dspmap_t* m) { return (m && m->ly.nr_valid) ? m->ly.nr_dist : nullptr; }
static int nearest_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.nr_valid, what,
                          "no nearest field, or the map or the cast grid it was built from has changed since (dspmap_build_nearest_field)");
}
extern "C" int dspmap_get_nearest_field(dspmap_t* m, int layer, int* near_out, float* dist_out) {
    if (!m) return DSPMAP_E_ARG;
    if (!near_out && !dist_out) return dspmap_fail(m, DSPMAP_E_ARG, "nearest field: both output arrays are NULL");
    if (layer < 0 || layer > m->d.T) return dspmap_fail(m, DSPMAP_E_ARG, "nearest field: layer %d outside [0, %d)", layer, m->d.T + 1);
    int rc = nearest_ready(m, "dspmap_get_nearest_field");
    if (rc != DSPMAP_OK) return rc;
    const size_t V = (size_t)m->d.v_glob;
    if (near_out && (rc = read_back(m, near_out, m->ly.nr_near + V * layer, sizeof(int) * V)) != DSPMAP_OK) return rc;
    if (dist_out && (rc = read_back(m, dist_out, m->ly.nr_dist + V * layer, sizeof(float) * V)) != DSPMAP_OK) return rc;
    return DSPMAP_OK;
}
static int nearest_query_check(dspmap* m, int n, const void* in, const void* out, int flags, float outside) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "nearest query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "nearest query", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    if (outside != outside) return dspmap_fail(m, DSPMAP_E_ARG, "nearest query: outside_value is NaN");
    return nearest_ready(m, "dspmap_query_nearest");
}
static int nearest_query_enqueue(dspmap* m, int n, const float4* dq, int flags, float outside, dspmap_nearest* dout) {
    const MapDims& d = m->d;
    NearQueryArgs a;
    a.org = origin_fill(m, flags);
    a.outside = outside;
    a.cx = -d.half_x + d.res * 0.5f; a.cy = -d.half_y + d.res * 0.5f; a.cz = -d.half_z + d.res * 0.5f;   // dspmap_voxel_center
    a.near = m->ly.nr_near; a.dist = m->ly.nr_dist;
    launch_nearest_query(dspmap_ctx_of(m), a, n, dq, dout);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_nearest(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, dspmap_nearest* out) {
    int rc = nearest_query_check(m, n, q, out, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, out, sizeof(dspmap_nearest) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = nearest_query_enqueue(m, n, (const float4*)s[0].dev, flags, outside, (dspmap_nearest*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_query_nearest_device(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, dspmap_nearest* out) {
    const int rc = nearest_query_check(m, n, q, out, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    return nearest_query_enqueue(m, n, (const float4*)q, flags, outside, out);
}

// --------------------------------------------------- segment casts (dspmap_cast.hip; semantics in include/dspmap.h)
extern "C" int dspmap_build_cast_grid(dspmap_t* m, float thr, int inflate_voxels, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (thr != thr) return dspmap_fail(m, DSPMAP_E_ARG, "cast grid: threshold is NaN");
    if (inflate_voxels < 0 || inflate_voxels > DSPMAP_CAST_MAX_INFLATE)
        return dspmap_fail(m, DSPMAP_E_ARG, "cast grid: inflate_voxels %d outside [0, %d]", inflate_voxels, DSPMAP_CAST_MAX_INFLATE);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "cast grid: unknown flags 0x%x", flags);
    const int rc = whole_map_check(m, "cast grid", "casts cross slabs");
    if (rc != DSPMAP_OK) return rc;
    const MapDims& d = m->d;
    const size_t words = (size_t)(d.T + 1) * grid_layer_words(d);
    if (words > 0x7fffffffull) return dspmap_fail(m, DSPMAP_E_STATE, "cast grid: %zu words exceed INT_MAX", words);
    READY(m);
    BENIGN(m);
    dspmap_layers_stale(m->ly, LAYERS_CAST_GRID_REBUILD);   // (with the arrival fields grown and the frontiers found in the grid this build replaces)
    if (!m->ly.cg_bits) {
        HIPCHK(m, hipMalloc(&m->ly.cg_bits, sizeof(u64) * words));
        HIPCHK(m, hipMalloc(&m->ly.cg_tmp, sizeof(u64) * words));
    }
    CastGridArgs a;
    a.thr = thr; a.r = inflate_voxels;
    a.fut_zero = m->fut_clear_pending ? 1 : 0;   // read, never changed (as the queries)
    a.L = d.T + 1;
    a.bits = m->ly.cg_bits; a.tmp = m->ly.cg_tmp;
    launch_cast_grid(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    m->ly.cg_valid = true;
    return DSPMAP_OK;
}
extern "C" const unsigned long long* dspmap_cast_grid_device(dspmap_t* m) { return (m && m->ly.cg_valid) ? m->ly.cg_bits : nullptr; }
static int cast_grid_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.cg_valid, what, "no cast grid, or the map has changed since it was built (dspmap_build_cast_grid)");
}
extern "C" int dspmap_get_cast_grid(dspmap_t* m, int layer, unsigned long long* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "cast grid: NULL output array");
    if (layer < 0 || layer > m->d.T) return dspmap_fail(m, DSPMAP_E_ARG, "cast grid: layer %d outside [0, %d)", layer, m->d.T + 1);
    const int rc = cast_grid_ready(m, "dspmap_get_cast_grid");
    if (rc != DSPMAP_OK) return rc;
    const size_t lw = grid_layer_words(m->d);
    return read_back(m, out, m->ly.cg_bits + lw * layer, sizeof(u64) * lw);
}
static int cast_check(dspmap* m, int n, const void* in, const void* out, int flags) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "cast", "segment", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "cast", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    return cast_grid_ready(m, "dspmap_cast_segments");
}
static CastArgs cast_args(const dspmap* m, int flags) {
    CastArgs a;
    a.org = origin_fill(m, flags);
    a.bits = m->ly.cg_bits;
    return a;
}
static int cast_enqueue(dspmap* m, int n, const dspmap_segment* ds, int flags, dspmap_cast_hit* dh) {
    launch_cast(dspmap_ctx_of(m), cast_args(m, flags), n, ds, dh);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_cast_segments(dspmap_t* m, int n, const dspmap_segment* seg, int flags, dspmap_cast_hit* out) {
    int rc = cast_check(m, n, seg, out, flags);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{seg, nullptr, sizeof(dspmap_segment) * (size_t)n}, {nullptr, out, sizeof(dspmap_cast_hit) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = cast_enqueue(m, n, (const dspmap_segment*)s[0].dev, flags, (dspmap_cast_hit*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_cast_segments_device(dspmap_t* m, int n, const dspmap_segment* seg, int flags, dspmap_cast_hit* out) {
    const int rc = cast_check(m, n, seg, out, flags);
    if (rc != DSPMAP_OK) return rc;
    return cast_enqueue(m, n, seg, flags, out);
}

// --------------------------------------------------- free boxes in the cast grid (dspmap_corridor.hip; semantics in include/dspmap.h)
static int box_check(dspmap* m, int n, const void* in, const int* max_grow, int flags, const void* out) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "grow boxes", "seed", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if (!max_grow) return dspmap_fail(m, DSPMAP_E_ARG, "grow boxes: NULL max_grow");
    for (int k = 0; k < 3; ++k)
        if (max_grow[k] < 0 || max_grow[k] > DSPMAP_BOX_MAX_GROW)
            return dspmap_fail(m, DSPMAP_E_ARG, "grow boxes: max_grow[%d] = %d outside [0, %d]", k, max_grow[k], DSPMAP_BOX_MAX_GROW);
    if ((rc = flags_check(m, "grow boxes", flags, DSPMAP_QUERY_WORLD | DSPMAP_BOX_WITH_CURRENT)) != DSPMAP_OK) return rc;
    if ((rc = whole_map_check(m, "grow boxes", "boxes cross slabs")) != DSPMAP_OK) return rc;
    return cast_grid_ready(m, "dspmap_grow_boxes");
}
static BoxArgs box_args(const dspmap* m, const int* max_grow, int flags) {
    BoxArgs a;
    a.org = origin_fill(m, flags);
    a.with_current = (flags & DSPMAP_BOX_WITH_CURRENT) ? 1 : 0;
    for (int k = 0; k < 3; ++k) a.grow[k] = max_grow[k];
    a.bits = m->ly.cg_bits;
    return a;
}
static int box_enqueue(dspmap* m, int n, const dspmap_segment* ds, const int* max_grow, int flags, dspmap_box* db) {
    launch_grow_boxes(dspmap_ctx_of(m), box_args(m, max_grow, flags), n, ds, db);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_grow_boxes(dspmap_t* m, int n, const dspmap_segment* seed, const int max_grow[3], int flags, dspmap_box* out) {
    int rc = box_check(m, n, seed, max_grow, flags, out);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{seed, nullptr, sizeof(dspmap_segment) * (size_t)n}, {nullptr, out, sizeof(dspmap_box) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = box_enqueue(m, n, (const dspmap_segment*)s[0].dev, max_grow, flags, (dspmap_box*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_grow_boxes_device(dspmap_t* m, int n, const dspmap_segment* seed, const int max_grow[3], int flags, dspmap_box* out) {
    const int rc = box_check(m, n, seed, max_grow, flags, out);
    if (rc != DSPMAP_OK) return rc;
    return box_enqueue(m, n, seed, max_grow, flags, out);
}

// --------------------------------------------------- arrival-time fields (dspmap_reach.hip; semantics in include/dspmap.h)
// the layer step n tests: the host twin of reach_layer (dspmap_reach.hip) -- the same fp32 operations, the k(t) of q_horizon
static int reach_layer_host(const MapDims& d, bool timed, float t_start, float step_seconds, int n) {
    if (!timed) return 0;
    volatile float prod = (float)n * step_seconds;   // (volatile: two roundings, whatever the host compiler would like to fuse)
    volatile float t = t_start + prod;
    const float tt = t;
    int k = d.T - 1;
    for (int j = d.T - 1; j >= 0; --j)
        if (d.pred_t[j] >= tt) k = j;
    return k + 1;
}
// the checks of both builds; `timeline`: dspmap_build_reach_timeline*, which adds the cap on the kept sets behind the other arguments
static int reach_build_check(dspmap* m, int n_fields, int n_src, const void* src, float t_start, float step_seconds, int max_steps, int flags,
                             bool timeline = false) {
    if (!m) return DSPMAP_E_ARG;
    if (n_fields < 1 || n_fields > DSPMAP_REACH_MAX_FIELDS)
        return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: n_fields %d outside [1, %d]", n_fields, DSPMAP_REACH_MAX_FIELDS);
    if (n_src < 0) return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: negative source count %d", n_src);
    if (n_src > 0 && !src) return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: NULL source array");
    if (t_start != t_start) return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: t_start is NaN");
    if (!(step_seconds >= 0.f && step_seconds < INFINITY))
        return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: step_seconds %g is NaN, negative or infinite", (double)step_seconds);
    if (max_steps < 1 || max_steps > DSPMAP_REACH_MAX_STEPS)
        return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: max_steps %d outside [1, %d]", max_steps, DSPMAP_REACH_MAX_STEPS);
    if (flags & ~(DSPMAP_QUERY_WORLD | DSPMAP_REACH_WITH_CURRENT | DSPMAP_REACH_DEVICE_SETS))
        return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: unknown flags 0x%x", flags);
    const unsigned long long cells = (unsigned long long)n_fields * (unsigned long long)m->d.v_glob;
    if (cells > 0x80000000ull) return dspmap_fail(m, DSPMAP_E_ARG, "reach fields: %d fields of %d cells exceed 2^31 cells", n_fields, m->d.v_glob);
    if (timeline) {   // (n_fields <= 64, max_steps + 1 <= 4097, a layer's words < 2^31: no overflow in 64 bits)
        const unsigned long long bytes = (unsigned long long)n_fields * (unsigned long long)(max_steps + 1) * grid_layer_words(m->d) * sizeof(u64);
        if (bytes > DSPMAP_REACH_TIMELINE_MAX_BYTES)
            return dspmap_fail(m, DSPMAP_E_ARG, "reach timeline: the sets of %d fields and %d steps take %llu bytes, more than "
                                                "DSPMAP_REACH_TIMELINE_MAX_BYTES = %llu", n_fields, max_steps + 1, bytes,
                               (unsigned long long)DSPMAP_REACH_TIMELINE_MAX_BYTES);
    }
    const int rc = whole_map_check(m, "reach fields", "a wavefront crosses slabs");
    if (rc != DSPMAP_OK) return rc;
    return cast_grid_ready(m, timeline ? "dspmap_build_reach_timeline" : "dspmap_build_reach_fields");
}
// the launch behind all four build entry points; src_dev may be NULL with n_src == 0.  keep: the timeline build, which also stores every
// step's set (a plain build replaces the fields a timeline belongs to, so it leaves none)
static int reach_build(dspmap* m, int n_fields, int n_src, const dspmap_reach_point* src_dev, float t_start, float step_seconds, int max_steps,
                       int flags, bool keep = false) {
    const MapDims& d = m->d;
    dspmap_layers_stale(m->ly, LAYERS_REACH_REBUILD);
    const size_t cells = (size_t)n_fields * d.v_glob, lw = grid_layer_words(d);
    const bool lds = 2 * sizeof(u64) * lw <= (size_t)REACH_LDS_BYTES && !(flags & DSPMAP_REACH_DEVICE_SETS);
    const size_t set_words = lds ? 0 : 2 * lw * (size_t)n_fields;
    const size_t hist_words = keep ? (size_t)n_fields * ((size_t)max_steps + 1) * lw : 0;
    if (cells > m->ly.rf_field_cells || set_words > m->ly.rf_sets_words || hist_words > m->ly.tl_hist_words || (keep && !m->ly.tl_last)) {   // grown only after the stream has drained (an earlier call may still read them)
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (!m->ly.rf_field) reach_init_device();
        int rc = layer_buf_grow(m, &m->ly.rf_field, &m->ly.rf_field_cells, cells);
        if (rc == DSPMAP_OK) rc = layer_buf_grow(m, &m->ly.rf_sets, &m->ly.rf_sets_words, set_words);
        if (rc == DSPMAP_OK) rc = layer_buf_grow(m, &m->ly.tl_hist, &m->ly.tl_hist_words, hist_words);
        if (rc != DSPMAP_OK) return rc;
        if (keep && !m->ly.tl_last) HIPCHK(m, hipMalloc(&m->ly.tl_last, sizeof(int) * DSPMAP_REACH_MAX_FIELDS));
    }
    ReachArgs a;
    a.org = origin_fill(m, flags);
    a.with_current = (flags & DSPMAP_REACH_WITH_CURRENT) ? 1 : 0;
    const bool timed = !(t_start < 0.f) && d.T > 0;
    a.timed = timed ? 1 : 0;
    a.t_start = t_start; a.step_seconds = step_seconds; a.max_steps = max_steps;
    const int l_last = reach_layer_host(d, timed, t_start, step_seconds, max_steps);
    int n_fix = max_steps;
    while (n_fix > 0 && reach_layer_host(d, timed, t_start, step_seconds, n_fix - 1) == l_last) --n_fix;
    a.n_fix = n_fix;
    a.n_fields = n_fields; a.n_src = n_src;
    a.bits = m->ly.cg_bits; a.field = m->ly.rf_field; a.sets = lds ? nullptr : m->ly.rf_sets;
    HIPCHK(m, hipMemsetAsync(m->ly.rf_field, 0xff, sizeof(unsigned short) * cells, m->stream));   // every value DSPMAP_REACH_UNREACHED
    launch_reach(dspmap_ctx_of(m), a, src_dev, keep ? m->ly.tl_hist : nullptr, keep ? m->ly.tl_last : nullptr);
    HIPCHK(m, hipGetLastError());
    m->ly.rf_n = n_fields;
    m->ly.rf_invariant = reach_layer_host(d, timed, t_start, step_seconds, 0) == l_last;
    m->ly.rf_storage[0] = lds ? n_fields : 0; m->ly.rf_storage[1] = lds ? 0 : n_fields;
    m->ly.rf_valid = true;
    if (keep) m->ly.tl_valid = true;
    m->ly.tl_max_steps = max_steps;
    return DSPMAP_OK;
}
// the synchronous entry points: the sources go through the query staging buffer
static int reach_build_host(dspmap* m, int n_fields, int n_src, const dspmap_reach_point* src, float t_start, float step_seconds, int max_steps,
                            int flags, bool keep) {
    int rc = reach_build_check(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags, keep);
    if (rc != DSPMAP_OK) return rc;
    StageSec s[1] = {{src, nullptr, sizeof(dspmap_reach_point) * (size_t)n_src}};   // (no sources: no section, the kernel gets NULL)
    if ((rc = stage_begin(m, s, 1)) != DSPMAP_OK) return rc;
    if ((rc = reach_build(m, n_fields, n_src, (const dspmap_reach_point*)s[0].dev, t_start, step_seconds, max_steps, flags, keep)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 1);
}
extern "C" int dspmap_build_reach_fields(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t_start, float step_seconds,
                                         int max_steps, int flags) {
    return reach_build_host(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags, false);
}
extern "C" int dspmap_build_reach_timeline(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t_start, float step_seconds,
                                           int max_steps, int flags) {
    return reach_build_host(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags, true);
}
extern "C" int dspmap_build_reach_timeline_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t_start,
                                                  float step_seconds, int max_steps, int flags) {
    const int rc = reach_build_check(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags, true);
    if (rc != DSPMAP_OK) return rc;
    return reach_build(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags, true);
}
extern "C" int dspmap_build_reach_fields_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t_start,
                                                float step_seconds, int max_steps, int flags) {
    const int rc = reach_build_check(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags);
    if (rc != DSPMAP_OK) return rc;
    return reach_build(m, n_fields, n_src, src, t_start, step_seconds, max_steps, flags);
}
extern "C" const unsigned short* dspmap_reach_fields_device(dspmap_t* m) { return (m && m->ly.rf_valid) ? m->ly.rf_field : nullptr; }
static int reach_ready(dspmap* m, const char* what) {
    const int rc = whole_map_check(m, what, "a wavefront crosses slabs");
    if (rc != DSPMAP_OK) return rc;
    return snapshot_ready(m, m->ly.rf_valid, what,
                          "no arrival fields, or the map or its cast grid has changed since they were built (dspmap_build_reach_fields)");
}
extern "C" int dspmap_get_reach_field(dspmap_t* m, int field, unsigned short* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "reach field: NULL output array");
    if (field < 0 || field >= DSPMAP_REACH_MAX_FIELDS) return dspmap_fail(m, DSPMAP_E_ARG, "reach field: field %d outside [0, %d)", field, DSPMAP_REACH_MAX_FIELDS);
    const int rc = reach_ready(m, "dspmap_get_reach_field");
    if (rc != DSPMAP_OK) return rc;
    if (field >= m->ly.rf_n) return dspmap_fail(m, DSPMAP_E_ARG, "reach field: field %d outside [0, %d), the fields of the last build", field, m->ly.rf_n);
    return read_back(m, out, m->ly.rf_field + (size_t)field * m->d.v_glob, sizeof(unsigned short) * (size_t)m->d.v_glob);
}
// the fields' timeline: valid while the fields it was built with are
static int reach_timeline_ready(dspmap* m, const char* what) {
    const int rc = whole_map_check(m, what, "a wavefront crosses slabs");
    if (rc != DSPMAP_OK) return rc;
    return snapshot_ready(m, m->ly.tl_valid, what,
                          "no timeline, or the map, its cast grid or the arrival fields have changed since it was built (dspmap_build_reach_timeline)");
}
extern "C" const unsigned long long* dspmap_reach_timeline_device(dspmap_t* m) {
    return (m && m->ly.tl_valid) ? (const unsigned long long*)m->ly.tl_hist : nullptr;
}
extern "C" int dspmap_reach_last_steps(dspmap_t* m, int* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "reach last steps: NULL output array");
    const int rc = reach_timeline_ready(m, "dspmap_reach_last_steps");
    if (rc != DSPMAP_OK) return rc;
    return read_back(m, out, m->ly.tl_last, sizeof(int) * (size_t)m->ly.rf_n);
}
extern "C" int dspmap_get_reach_sets(dspmap_t* m, int field, int first_step, int n_steps, unsigned long long* out) {
    if (!m) return DSPMAP_E_ARG;
    if (field < 0 || field >= DSPMAP_REACH_MAX_FIELDS) return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: field %d outside [0, %d)", field, DSPMAP_REACH_MAX_FIELDS);
    if (first_step < 0) return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: negative first_step %d", first_step);
    if (n_steps < 0) return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: negative n_steps %d", n_steps);
    if (first_step > DSPMAP_REACH_MAX_STEPS + 1 || n_steps > DSPMAP_REACH_MAX_STEPS + 1 - first_step)
        return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: steps [%d, %d + %d) outside [0, %d]", first_step, first_step, n_steps, DSPMAP_REACH_MAX_STEPS);
    if (n_steps > 0 && !out) return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: NULL output array with n_steps %d", n_steps);
    const int rc = reach_timeline_ready(m, "dspmap_get_reach_sets");
    if (rc != DSPMAP_OK) return rc;
    if (field >= m->ly.rf_n) return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: field %d outside [0, %d), the fields of the last build", field, m->ly.rf_n);
    if (first_step + n_steps > m->ly.tl_max_steps + 1)
        return dspmap_fail(m, DSPMAP_E_ARG, "reach sets: steps [%d, %d) outside [0, %d], the steps of the last build", first_step, first_step + n_steps,
                           m->ly.tl_max_steps);
    if (n_steps == 0) return DSPMAP_OK;
    int last = 0;   // the field's last executed step: a later one repeats its row
    HIPCHK(m, hipMemcpyAsync(&last, m->ly.tl_last + field, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (last < 0 || last > m->ly.tl_max_steps) return dspmap_fail(m, DSPMAP_E_DEVICE, "reach sets: field %d reports last step %d outside [0, %d]", field, last, m->ly.tl_max_steps);
    const size_t lw = grid_layer_words(m->d);
    const u64* rows = m->ly.tl_hist + (size_t)field * ((size_t)m->ly.tl_max_steps + 1) * lw;
    const int n_own = first_step > last ? 0 : (first_step + n_steps - 1 > last ? last - first_step + 1 : n_steps);   // rows the build wrote
    if (n_own > 0) HIPCHK(m, hipMemcpyAsync(out, rows + (size_t)first_step * lw, sizeof(u64) * lw * (size_t)n_own, hipMemcpyDeviceToHost, m->stream));
    for (int k = n_own; k < n_steps; ++k)
        HIPCHK(m, hipMemcpyAsync(out + (size_t)k * lw, rows + (size_t)last * lw, sizeof(u64) * lw, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return DSPMAP_OK;
}
// the paths through the fields: dspmap_reach_paths*, dspmap_reach_timeline_paths* and dspmap_cost_paths* are one check, one enqueue and one
// host / device pair; `what` and `out_name` keep every message what its entry point always said
enum PathKind { PATHS_REACH, PATHS_TIMELINE, PATHS_COST };
static int cost_ready(dspmap* m, const char* what);   // (with the cost fields, below)
static int paths_args_check(dspmap* m, const char* what, const char* out_name, int n, const void* start, int max_len, int flags, const void* steps_out,
                            const void* cells_out) {
    if (!m) return DSPMAP_E_ARG;
    if (n < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative start count %d", what, n);
    if (max_len < 0 || max_len > DSPMAP_REACH_MAX_STEPS + 1)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: max_len %d outside [0, %d]", what, max_len, DSPMAP_REACH_MAX_STEPS + 1);
    if (n > 0 && (!start || !steps_out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL start or %s array", what, out_name);
    if (n > 0 && max_len > 0 && !cells_out) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL cells_out array with max_len %d", what, max_len);
    const int rc = flags_check(m, what, flags, DSPMAP_QUERY_WORLD);
    if (rc != DSPMAP_OK) return rc;
    if ((unsigned long long)n * (unsigned long long)max_len > 0x80000000ull)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: %d paths of %d cells exceed 2^31 cells", what, n, max_len);
    return DSPMAP_OK;
}
// ... then the state: the plain reach paths need time-invariant fields, the timeline's paths the sets a timeline build kept, the cost paths
// the cost fields
static int paths_check(dspmap* m, PathKind kind, int n, const void* start, int max_len, int flags, const void* steps_out, const void* cells_out) {
    const bool cost = kind == PATHS_COST;
    int rc = paths_args_check(m, cost ? "cost paths" : "reach paths", cost ? "cost_out" : "steps_out", n, start, max_len, flags, steps_out, cells_out);
    if (rc != DSPMAP_OK) return rc;
    if (cost) return cost_ready(m, "dspmap_cost_paths");
    if (kind == PATHS_TIMELINE) return reach_timeline_ready(m, "dspmap_reach_timeline_paths");
    if ((rc = reach_ready(m, "dspmap_reach_paths")) != DSPMAP_OK) return rc;
    if (!m->ly.rf_invariant)
        return dspmap_fail(m, DSPMAP_E_STATE, "reach paths: the fields of the last build are not time-invariant (the tested layer changed "
                                              "during the steps): first arrivals alone do not determine a path");
    return DSPMAP_OK;
}
static int paths_enqueue(dspmap* m, PathKind kind, int n, const dspmap_reach_point* ds, int max_len, int flags, int* dt, int* dc) {
    if (kind == PATHS_TIMELINE) {
        ReachTimelinePathArgs a;
        a.org = origin_fill(m, flags);
        a.n_fields = m->ly.rf_n; a.max_len = max_len; a.max_steps = m->ly.tl_max_steps;
        a.field = m->ly.rf_field; a.hist = m->ly.tl_hist; a.last = m->ly.tl_last;
        launch_reach_timeline_paths(dspmap_ctx_of(m), a, n, ds, dt, dc);
    } else {
        const bool cost = kind == PATHS_COST;
        FieldPathArgs a;
        a.org = origin_fill(m, flags);
        a.n_fields = cost ? m->ly.cf_n : m->ly.rf_n; a.max_len = max_len;
        a.field = cost ? m->ly.cf_field : m->ly.rf_field;
        a.weight = cost ? m->ly.cf_weight : nullptr;
        launch_field_paths(dspmap_ctx_of(m), a, cost, n, ds, dt, dc);
    }
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
// the host entry points (max_len == 0: no cells section, the kernel gets NULL) ...
static int paths_host(dspmap* m, PathKind kind, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out, int* cells_out) {
    int rc = paths_check(m, kind, n, start, max_len, flags, steps_out, cells_out);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[3] = {{start, nullptr, sizeof(dspmap_reach_point) * (size_t)n}, {nullptr, steps_out, sizeof(int) * (size_t)n},
                     {nullptr, cells_out, sizeof(int) * (size_t)n * max_len}};
    if ((rc = stage_begin(m, s, 3)) != DSPMAP_OK) return rc;
    if ((rc = paths_enqueue(m, kind, n, (const dspmap_reach_point*)s[0].dev, max_len, flags, (int*)s[1].dev, (int*)s[2].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 3);
}
// ... and the stream-ordered ones
static int paths_device(dspmap* m, PathKind kind, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out, int* cells_out) {
    const int rc = paths_check(m, kind, n, start, max_len, flags, steps_out, cells_out);
    if (rc != DSPMAP_OK) return rc;
    return paths_enqueue(m, kind, n, start, max_len, flags, steps_out, cells_out);
}
extern "C" int dspmap_reach_paths(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out, int* cells_out) {
    return paths_host(m, PATHS_REACH, n, start, max_len, flags, steps_out, cells_out);
}
extern "C" int dspmap_reach_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out, int* cells_out) {
    return paths_device(m, PATHS_REACH, n, start, max_len, flags, steps_out, cells_out);
}
extern "C" int dspmap_reach_timeline_paths(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out,
                                           int* cells_out) {
    return paths_host(m, PATHS_TIMELINE, n, start, max_len, flags, steps_out, cells_out);
}
extern "C" int dspmap_reach_timeline_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* steps_out,
                                                  int* cells_out) {
    return paths_device(m, PATHS_TIMELINE, n, start, max_len, flags, steps_out, cells_out);
}
extern "C" int dspmap_cost_paths(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* cost_out, int* cells_out) {
    return paths_host(m, PATHS_COST, n, start, max_len, flags, cost_out, cells_out);
}
extern "C" int dspmap_cost_paths_device(dspmap_t* m, int n, const dspmap_reach_point* start, int max_len, int flags, int* cost_out, int* cells_out) {
    return paths_device(m, PATHS_COST, n, start, max_len, flags, cost_out, cells_out);
}
// --------------------------------------------------- shortened paths (dspmap_shorten.hip; semantics in include/dspmap.h)
// needs the cast grid only: the paths may come from a reach snapshot, from a stale one or from the caller
static int shorten_check(dspmap* m, int n, int max_len, const void* steps, const void* cells, float t_start, float step_seconds, int window,
                         int max_seg, int flags, const void* info, const void* seg, const void* end) {
    if (!m) return DSPMAP_E_ARG;
    if (n < 0) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: negative path count %d", n);
    if (max_len < 1 || max_len > DSPMAP_REACH_MAX_STEPS + 1)
        return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: max_len %d outside [1, %d]", max_len, DSPMAP_REACH_MAX_STEPS + 1);
    if (window < 1 || window > DSPMAP_SHORTEN_MAX_WINDOW)
        return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: window %d outside [1, %d]", window, DSPMAP_SHORTEN_MAX_WINDOW);
    if (max_seg < 0) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: negative max_seg %d", max_seg);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: unknown flags 0x%x", flags);
    if (t_start != t_start) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: t_start is NaN");
    if (!(step_seconds >= 0.f && step_seconds < INFINITY))
        return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: step_seconds %g is NaN, negative or infinite", (double)step_seconds);
    if (n > 0 && (!steps || !cells || !info)) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: NULL steps, cells or info array");
    if (n > 0 && max_seg > 0 && (!seg || !end)) return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: NULL seg_out or end_out array with max_seg %d", max_seg);
    if ((unsigned long long)n * (unsigned long long)max_len > 0x80000000ull)
        return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: %d paths of %d cells exceed 2^31 cells", n, max_len);
    if ((unsigned long long)n * (unsigned long long)max_seg > 0x80000000ull)
        return dspmap_fail(m, DSPMAP_E_ARG, "shorten paths: %d paths of %d segments exceed 2^31 segments", n, max_seg);
    const int rc = whole_map_check(m, "shorten paths", "casts cross slabs");
    if (rc != DSPMAP_OK) return rc;
    return cast_grid_ready(m, "dspmap_shorten_paths");
}
static int shorten_enqueue(dspmap* m, int n, int max_len, const int* steps, const int* cells, float t_start, float step_seconds, int window, int max_seg,
                           dspmap_path_info* info, dspmap_segment* seg, int* end) {
    const MapDims& d = m->d;
    ShortenArgs a;
    a.cx = -d.half_x + d.res * 0.5f; a.cy = -d.half_y + d.res * 0.5f; a.cz = -d.half_z + d.res * 0.5f;   // dspmap_voxel_center
    a.timed = (!(t_start < 0.f) && d.T > 0) ? 1 : 0;
    a.t_start = t_start; a.step_seconds = step_seconds;
    a.max_len = max_len; a.window = window; a.max_seg = max_seg;
    a.bits = m->ly.cg_bits;
    launch_shorten(dspmap_ctx_of(m), a, n, steps, cells, info, seg, end);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_shorten_paths(dspmap_t* m, int n, int max_len, const int* steps, const int* cells, float t_start, float step_seconds, int window,
                                    int max_seg, int flags, dspmap_path_info* info_out, dspmap_segment* seg_out, int* end_out) {
    int rc = shorten_check(m, n, max_len, steps, cells, t_start, step_seconds, window, max_seg, flags, info_out, seg_out, end_out);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    const size_t ns = (size_t)n * max_seg;   // (max_seg == 0: no segment sections, the kernel gets NULL)
    StageSec s[5] = {{steps, nullptr, sizeof(int) * (size_t)n}, {cells, nullptr, sizeof(int) * (size_t)n * max_len},
                     {nullptr, info_out, sizeof(dspmap_path_info) * (size_t)n}, {nullptr, seg_out, sizeof(dspmap_segment) * ns},
                     {nullptr, end_out, sizeof(int) * ns}};
    if ((rc = stage_begin(m, s, 5)) != DSPMAP_OK) return rc;
    if ((rc = shorten_enqueue(m, n, max_len, (const int*)s[0].dev, (const int*)s[1].dev, t_start, step_seconds, window, max_seg,
                              (dspmap_path_info*)s[2].dev, (dspmap_segment*)s[3].dev, (int*)s[4].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 5);
}
extern "C" int dspmap_shorten_paths_device(dspmap_t* m, int n, int max_len, const int* steps, const int* cells, float t_start, float step_seconds,
                                           int window, int max_seg, int flags, dspmap_path_info* info_out, dspmap_segment* seg_out, int* end_out) {
    const int rc = shorten_check(m, n, max_len, steps, cells, t_start, step_seconds, window, max_seg, flags, info_out, seg_out, end_out);
    if (rc != DSPMAP_OK) return rc;
    return shorten_enqueue(m, n, max_len, steps, cells, t_start, step_seconds, window, max_seg, info_out, seg_out, end_out);
}

extern "C" int dspmap_debug_reach_storage(dspmap_t* m, long long out[2]) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "reach storage: NULL output array");
    out[0] = m->ly.rf_storage[0]; out[1] = m->ly.rf_storage[1];
    return DSPMAP_OK;
}
// test hook: all L layers of the VALID cast grid are replaced by the caller's words
extern "C" int dspmap_debug_set_cast_grid(dspmap_t* m, const unsigned long long* words) {
    if (!m) return DSPMAP_E_ARG;
    if (!words) return dspmap_fail(m, DSPMAP_E_ARG, "set cast grid: NULL word array");
    const MapDims& d = m->d;
    const size_t nw = grid_row_words(d), total = (size_t)(d.T + 1) * grid_layer_words(d);
    if (d.nx & 63) {
        const unsigned long long pad = ~0ull << (d.nx & 63);
        for (size_t i = nw - 1; i < total; i += nw)
            if (words[i] & pad) return dspmap_fail(m, DSPMAP_E_ARG, "set cast grid: word %zu has a bit set at x >= nx", i);
    }
    int rc = whole_map_check(m, "set cast grid", "");
    if (rc != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, "dspmap_debug_set_cast_grid")) != DSPMAP_OK) return rc;
    dspmap_layers_stale(m->ly, LAYERS_CAST_GRID_CHANGED);
    HIPCHK(m, hipMemcpyAsync(m->ly.cg_bits, words, sizeof(u64) * total, hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));   // (the caller's array is free again)
    return DSPMAP_OK;
}

// --------------------------------------------------- occupancy forecast at caller-chosen times (dspmap_forecast.hip; semantics in include/dspmap.h)
static_assert(FORECAST_MAX_TIMES == DSPMAP_FORECAST_MAX_TIMES, "ForecastArgs holds DSPMAP_FORECAST_MAX_TIMES times");
extern "C" int dspmap_build_forecast(dspmap_t* m, int n_times, const float* times, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (n_times < 1 || n_times > DSPMAP_FORECAST_MAX_TIMES)
        return dspmap_fail(m, DSPMAP_E_ARG, "forecast: n_times %d outside [1, %d]", n_times, DSPMAP_FORECAST_MAX_TIMES);
    if (!times) return dspmap_fail(m, DSPMAP_E_ARG, "forecast: NULL times array");
    for (int j = 0; j < n_times; ++j) {
        if (!(times[j] >= 0.f && times[j] < INFINITY))
            return dspmap_fail(m, DSPMAP_E_ARG, "forecast: times[%d] = %g is NaN, infinite or negative", j, (double)times[j]);
        if (j > 0 && !(times[j] > times[j - 1]))
            return dspmap_fail(m, DSPMAP_E_ARG, "forecast: times[%d] = %g is not greater than times[%d] = %g", j, (double)times[j], j - 1, (double)times[j - 1]);
    }
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "forecast: unknown flags 0x%x", flags);
    if ((unsigned long long)n_times * (unsigned long long)m->d.v_glob >= 0x80000000ull)
        return dspmap_fail(m, DSPMAP_E_ARG, "forecast: %d layers of %d cells reach 2^31 cells", n_times, m->d.v_glob);
    const int rc = whole_map_check(m, "forecast", "particles cross slabs");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    const MapDims& d = m->d;
    dspmap_layers_stale(m->ly, LAYERS_FORECAST_REBUILD);
    if (n_times > m->ly.fc_cap) {   // grown only after the stream has drained (an earlier call may still read them)
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (m->ly.fc_field) { HIPCHK(m, hipFree(m->ly.fc_field)); m->ly.fc_field = nullptr; }
        if (m->ly.fc_acc) { HIPCHK(m, hipFree(m->ly.fc_acc)); m->ly.fc_acc = nullptr; }
        m->ly.fc_cap = 0;
        HIPCHK(m, hipMalloc(&m->ly.fc_field, sizeof(float) * (size_t)n_times * d.v_glob));
        HIPCHK(m, hipMalloc(&m->ly.fc_acc, sizeof(u64) * (size_t)(n_times + 1) * d.v_loc));
        m->ly.fc_cap = n_times;
    }
    ForecastArgs a;
    a.n = n_times;
    for (int j = 0; j < FORECAST_MAX_TIMES; ++j) a.t[j] = j < n_times ? times[j] : 0.f;
    a.dyn = m->ly.fc_acc; a.stat = m->ly.fc_acc + (size_t)n_times * d.v_loc; a.out = m->ly.fc_field;
    HIPCHK(m, hipMemsetAsync(m->ly.fc_acc, 0, sizeof(u64) * (size_t)(n_times + 1) * d.v_loc, m->stream));   // dyn and stat: one allocation
    launch_forecast(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    m->ly.fc_n = n_times;
    for (int j = 0; j < n_times; ++j) m->ly.fc_t[j] = times[j];
    m->ly.fc_valid = true;
    return DSPMAP_OK;
}
extern "C" const float* dspmap_forecast_device(dspmap_t* m) { return (m && m->ly.fc_valid) ? m->ly.fc_field : nullptr; }
static int forecast_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.fc_valid, what, "no forecast, or the map has changed since it was built (dspmap_build_forecast)");
}
extern "C" int dspmap_forecast_times(dspmap_t* m, float* times_out, int cap) {
    if (!m) return DSPMAP_E_ARG;
    if (cap > 0 && !times_out) return dspmap_fail(m, DSPMAP_E_ARG, "forecast times: NULL output array");
    const int rc = forecast_ready(m, "dspmap_forecast_times");
    if (rc != DSPMAP_OK) return rc;
    for (int j = 0; j < m->ly.fc_n && j < cap; ++j) times_out[j] = m->ly.fc_t[j];
    return m->ly.fc_n;
}
extern "C" int dspmap_get_forecast(dspmap_t* m, int layer, float* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "forecast: NULL output array");
    if (layer < 0 || layer >= DSPMAP_FORECAST_MAX_TIMES) return dspmap_fail(m, DSPMAP_E_ARG, "forecast: layer %d outside [0, %d)", layer, DSPMAP_FORECAST_MAX_TIMES);
    const int rc = forecast_ready(m, "dspmap_get_forecast");
    if (rc != DSPMAP_OK) return rc;
    if (layer >= m->ly.fc_n) return dspmap_fail(m, DSPMAP_E_ARG, "forecast: layer %d outside [0, %d), the layers of the last build", layer, m->ly.fc_n);
    const size_t V = (size_t)m->d.v_glob;
    return read_back(m, out, m->ly.fc_field + V * layer, sizeof(float) * V);
}
static int forecast_query_check(dspmap* m, int n, const void* in, const void* out, int flags, float outside) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "forecast query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "forecast query", flags, DSPMAP_QUERY_WORLD | DSPMAP_FORECAST_LERP)) != DSPMAP_OK) return rc;
    if (outside != outside) return dspmap_fail(m, DSPMAP_E_ARG, "forecast query: outside_value is NaN");
    return forecast_ready(m, "dspmap_query_forecast");
}
static ForecastQueryArgs forecast_query_args(const dspmap* m, int flags, float outside) {
    ForecastQueryArgs a;
    a.org = origin_fill(m, flags);
    a.lerp = (flags & DSPMAP_FORECAST_LERP) ? 1 : 0;
    a.outside = outside;
    a.n = m->ly.fc_n;
    for (int j = 0; j < FORECAST_MAX_TIMES; ++j) a.t[j] = j < m->ly.fc_n ? m->ly.fc_t[j] : 0.f;
    a.field = m->ly.fc_field;
    return a;
}
static int forecast_query_enqueue(dspmap* m, int n, const float4* dq, int flags, float outside, float* dout) {
    launch_forecast_query(dspmap_ctx_of(m), forecast_query_args(m, flags, outside), n, dq, dout);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_forecast(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, float* out) {
    int rc = forecast_query_check(m, n, q, out, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, out, sizeof(float) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = forecast_query_enqueue(m, n, (const float4*)s[0].dev, flags, outside, (float*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_query_forecast_device(dspmap_t* m, int n, const dspmap_query* q, int flags, float outside, float* out) {
    const int rc = forecast_query_check(m, n, q, out, flags, outside);
    if (rc != DSPMAP_OK) return rc;
    return forecast_query_enqueue(m, n, (const float4*)q, flags, outside, out);
}

// --------------------------------------------------- known-space layer (dspmap_known.hip; semantics in include/dspmap.h)
// the window of the current position: lattice index k0 of map voxel 0 and the offset o of that cell's centre from the sensor, per axis, in
// double from the floats cur_pos and res (dspmap.h states the arithmetic; tests/known_ref.py restates it)
static int known_window(dspmap* m, long long k0[3], float o[3]) {
    const int n[3] = {m->d.nx, m->d.ny, m->d.nz};
    const double res = (double)m->d.res;
    for (int a = 0; a < 3; ++a) {
        const double cur = (double)m->cur_pos[a];
        const double g = cur / res - (double)n[a] / 2.0;
        if (!(fabs(g) < 4.0e15))   // (also NaN: dspmap_set_current_position takes any float)
            return dspmap_fail(m, DSPMAP_E_STATE, "known space: the current position %g on axis %d is not finite or beyond 4e15 cells", cur, a);
        k0[a] = (long long)floor(g + 0.5);
        o[a] = (float)(((double)k0[a] + 0.5) * res - cur);
    }
    return DSPMAP_OK;
}
static int known_slot(long long k, int n) { const long long r = k % n; return (int)(r < 0 ? r + n : r); }
// everything forgotten (dspmap_known_reset, dspmap_clear_state, dspmap_load_checkpoint); a handle without a layer has nothing to forget
int dspmap_known_forget(dspmap* m) {
    m->ly.kn_integrated = false;
    dspmap_layers_stale(m->ly, LAYERS_KNOWN_CHANGED);
    if (m->ly.kn_stamp) HIPCHK(m, hipMemsetAsync(m->ly.kn_stamp, 0, sizeof(unsigned) * (size_t)m->d.v_glob, m->stream));
    return DSPMAP_OK;
}
// FIRST thing in every entry point that reads or writes the layer: move the window to the current position.  The lattice cells that entered
// it since the last synchronisation are reset to "never" on the stream (their slots held the cells that left on the other side); a shift of
// n or more cells on an axis resets everything.  Fills the kernels' arguments.
static int known_sync(dspmap* m, KnownArgs* a) {
    long long k0[3];
    float o[3];
    const int rc = known_window(m, k0, o);
    if (rc != DSPMAP_OK) return rc;
    const MapDims& d = m->d;
    const int n[3] = {d.nx, d.ny, d.nz};
    if (m->ly.kn_stamp && (k0[0] != m->ly.kn_k0[0] || k0[1] != m->ly.kn_k0[1] || k0[2] != m->ly.kn_k0[2])) {
        int s0[3] = {0, 0, 0}, cnt[3] = {0, 0, 0};
        bool all = false;
        for (int ax = 0; ax < 3; ++ax) {
            const long long delta = k0[ax] - m->ly.kn_k0[ax];
            if (delta >= n[ax] || -delta >= n[ax]) { all = true; break; }
            // delta > 0: the cells [old + n, new + n) enter, delta < 0: the cells [new, old)
            if (delta > 0) { s0[ax] = known_slot(m->ly.kn_k0[ax], n[ax]); cnt[ax] = (int)delta; }
            else if (delta < 0) { s0[ax] = known_slot(k0[ax], n[ax]); cnt[ax] = (int)-delta; }
        }
        if (all) HIPCHK(m, hipMemsetAsync(m->ly.kn_stamp, 0, sizeof(unsigned) * (size_t)d.v_glob, m->stream));
        else launch_known_clear(d, m->stream, m->ly.kn_stamp, s0, cnt);
        HIPCHK(m, hipGetLastError());
    }
    for (int ax = 0; ax < 3; ++ax) m->ly.kn_k0[ax] = k0[ax];
    a->stamp = m->ly.kn_stamp;
    a->bx = known_slot(k0[0], d.nx); a->by = known_slot(k0[1], d.ny); a->bz = known_slot(k0[2], d.nz);
    a->ox = o[0]; a->oy = o[1]; a->oz = o[2];
    a->max_range = INFINITY;
    a->occl_margin = m->fp.occl_margin;
    a->now = (unsigned)m->update_counter;
    return DSPMAP_OK;
}
static int known_whole_map(dspmap* m, const char* what) { return whole_map_check(m, what, "the sensor's view crosses slabs"); }
extern "C" int dspmap_known_integrate(dspmap_t* m, float max_range, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (!(max_range > 0.f)) return dspmap_fail(m, DSPMAP_E_ARG, "known space: max_range %g is NaN or not positive", (double)max_range);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "known space: unknown flags 0x%x", flags);
    int rc = known_whole_map(m, "dspmap_known_integrate");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (m->update_counter < 1)
        return dspmap_fail(m, DSPMAP_E_STATE, "known space: no frame has been accepted yet, there is no view to integrate (dspmap_update)");
    dspmap_layers_stale(m->ly, LAYERS_KNOWN_CHANGED);
    const bool fresh = !m->ly.kn_stamp;
    if (fresh) {
        HIPCHK(m, hipMalloc(&m->ly.kn_stamp, sizeof(unsigned) * (size_t)m->d.v_glob));
        HIPCHK(m, hipMemsetAsync(m->ly.kn_stamp, 0, sizeof(unsigned) * (size_t)m->d.v_glob, m->stream));
    }
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) {
        if (fresh) { (void)hipStreamSynchronize(m->stream); (void)hipFree(m->ly.kn_stamp); m->ly.kn_stamp = nullptr; }
        return rc;
    }
    a.max_range = max_range;
    launch_known_integrate(m->d, m->s, m->stream, a, m->n_cu);
    HIPCHK(m, hipGetLastError());
    m->ly.kn_integrated = true;
    return DSPMAP_OK;
}
extern "C" int dspmap_known_reset(dspmap_t* m) {
    READY(m);
    BENIGN(m);
    return dspmap_known_forget(m);
}
extern "C" int dspmap_get_known(dspmap_t* m, int* age_out) {
    if (!m) return DSPMAP_E_ARG;
    if (!age_out) return dspmap_fail(m, DSPMAP_E_ARG, "known space: NULL output array");
    int rc = known_whole_map(m, "dspmap_get_known");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    const size_t V = (size_t)m->d.v_glob;
    if (!m->ly.kn_stamp) {   // never integrated: nothing allocated, nothing known
        for (size_t i = 0; i < V; ++i) age_out[i] = -1;
        return DSPMAP_OK;
    }
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    StageSec s[1] = {{nullptr, age_out, sizeof(int) * V}};
    if ((rc = stage_begin(m, s, 1)) != DSPMAP_OK) return rc;
    launch_known_ages(m->d, m->stream, a, (int*)s[0].dev);
    HIPCHK(m, hipGetLastError());
    return stage_end(m, s, 1);
}
static int known_query_check(dspmap* m, int n, const void* in, const void* out, int flags) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "known query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "known query", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    return known_whole_map(m, "dspmap_query_known");
}
// (the caller has synchronised the layer: known_sync queues work of its own, in front of the staging copies)
static int known_query_enqueue(dspmap* m, const KnownArgs& a, int n, const float4* dq, int flags, int* dout) {
    launch_known_query(m->d, m->stream, a, origin_fill(m, flags), n, dq, dout);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_known(dspmap_t* m, int n, const dspmap_query* q, int flags, int* age_out) {
    int rc = known_query_check(m, n, q, age_out, flags);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (n == 0) return DSPMAP_OK;
    if (!m->ly.kn_stamp) {
        for (int i = 0; i < n; ++i) age_out[i] = -1;
        return DSPMAP_OK;
    }
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    StageSec s[2] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, age_out, sizeof(int) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = known_query_enqueue(m, a, n, (const float4*)s[0].dev, flags, (int*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_query_known_device(dspmap_t* m, int n, const dspmap_query* q, int flags, int* age_out) {
    int rc = known_query_check(m, n, q, age_out, flags);
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if (n == 0) return DSPMAP_OK;
    if (!m->ly.kn_stamp) {   // never integrated: every byte 0xff is the int -1
        HIPCHK(m, hipMemsetAsync(age_out, 0xff, sizeof(int) * (size_t)n, m->stream));
        return DSPMAP_OK;
    }
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    return known_query_enqueue(m, a, n, (const float4*)q, flags, age_out);
}
extern "C" int dspmap_mask_cast_grid(dspmap_t* m, int max_age, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (max_age < 0) return dspmap_fail(m, DSPMAP_E_ARG, "mask cast grid: negative max_age %d", max_age);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "mask cast grid: unknown flags 0x%x", flags);
    int rc = cast_grid_ready(m, "dspmap_mask_cast_grid");
    if (rc != DSPMAP_OK) return rc;
    if (!m->ly.kn_stamp || !m->ly.kn_integrated)
        return dspmap_fail(m, DSPMAP_E_STATE, "mask cast grid: no frame has been integrated into the known-space layer (dspmap_known_integrate)");
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    dspmap_layers_stale(m->ly, LAYERS_CAST_GRID_CHANGED);   // (arrival fields were grown in the grid as it was, frontiers found in it)
    launch_known_mask(m->d, m->stream, a, max_age, m->d.T + 1, m->ly.cg_bits);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_known_stats(dspmap_t* m, int max_age, long long out[2]) {
    if (!m) return DSPMAP_E_ARG;
    if (max_age < 0) return dspmap_fail(m, DSPMAP_E_ARG, "known stats: negative max_age %d", max_age);
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "known stats: NULL output array");
    int rc = known_whole_map(m, "dspmap_known_stats");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    out[0] = out[1] = 0;
    if (!m->ly.kn_stamp) return DSPMAP_OK;
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    u64 sums[2] = {0, 0};
    StageSec s[1] = {{nullptr, sums, sizeof(sums)}};
    if ((rc = stage_begin(m, s, 1)) != DSPMAP_OK) return rc;
    HIPCHK(m, hipMemsetAsync(s[0].dev, 0, sizeof(sums), m->stream));
    launch_known_count(m->d, m->stream, a, max_age, (u64*)s[0].dev);
    HIPCHK(m, hipGetLastError());
    if ((rc = stage_end(m, s, 1)) != DSPMAP_OK) return rc;
    out[0] = (long long)sums[0]; out[1] = (long long)sums[1];
    return DSPMAP_OK;
}

// --------------------------------------------------- scores of candidate viewpoints (dspmap_view.hip; semantics in include/dspmap.h)
// the table of unrotated central directions, once per handle: (1, tan alpha_h, tan beta_v) / |.| in double, rounded to fp32
static int view_dirs(dspmap* m) {
    if (m->ly.vw_dirs0) return DSPMAP_OK;
    const MapDims& d = m->d;
    std::vector<float> t((size_t)d.np * 3);
    const double step = (double)m->cfg.angle_resolution * 3.14159265358979323846 / 180.0;
    for (int h = 0; h < d.np_h; ++h)
        for (int v = 0; v < d.np_v; ++v) {
            const double y = tan(((double)h - (double)d.np_h / 2.0 + 0.5) * step), z = tan(-((double)v - (double)d.np_v / 2.0 + 0.5) * step);
            const double len = sqrt(1.0 + y * y + z * z);
            float* o = &t[3 * ((size_t)h * d.np_v + v)];
            o[0] = (float)(1.0 / len); o[1] = (float)(y / len); o[2] = (float)(z / len);
        }
    float* dev = nullptr;
    HIPCHK(m, hipMalloc(&dev, sizeof(float) * t.size()));
    const hipError_t e = hipMemcpy(dev, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice);   // (synchronous: t is a local)
    if (e != hipSuccess) { (void)hipFree(dev); HIPCHK(m, e); }
    m->ly.vw_dirs0 = dev;
    return DSPMAP_OK;
}
static void view_args_geometry(const dspmap* m, ViewArgs* a, int flags) {
    const MapDims& d = m->d;
    a->org = origin_fill(m, flags);
    a->cx = -d.half_x + d.res * 0.5f; a->cy = -d.half_y + d.res * 0.5f; a->cz = -d.half_z + d.res * 0.5f;   // dspmap_voxel_center
    a->dirs0 = m->ly.vw_dirs0;
    a->reach = d.res * (float)(d.nx + d.ny + d.nz);
}
// the argument and state rules of every scoring entry point, in dspmap_grow_boxes' order; then the layer synchronised and the arguments filled
static int view_check(dspmap* m, int n, const void* in, int max_age, int flags, const void* out, const char* what) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, what, "view", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if (max_age < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative max_age %d", what, max_age);
    if ((rc = flags_check(m, what, flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    if ((rc = whole_map_check(m, what, "a view crosses slabs")) != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, what)) != DSPMAP_OK) return rc;
    if (!m->ly.kn_stamp || !m->ly.kn_integrated)
        return dspmap_fail(m, DSPMAP_E_STATE, "%s: no frame has been integrated into the known-space layer (dspmap_known_integrate)", what);
    return DSPMAP_OK;
}
static int view_args(dspmap* m, int max_age, int flags, ViewArgs* a) {
    int rc = view_dirs(m);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = known_sync(m, &a->kn)) != DSPMAP_OK) return rc;
    view_args_geometry(m, a, flags);
    a->bits = m->ly.cg_bits;
    a->max_age = max_age;
    return DSPMAP_OK;
}
// (the caller has filled the arguments: view_args synchronises the known-space layer, in front of the staging copies.)  The kernel adds
// into the scores, so they are zeroed first
static int view_score_enqueue(dspmap* m, const ViewArgs& a, int n, const dspmap_view* dv, dspmap_view_score* ds) {
    HIPCHK(m, hipMemsetAsync(ds, 0, sizeof(dspmap_view_score) * (size_t)n, m->stream));
    launch_view_score(m->d, m->s, m->stream, a, n, view_chunks(m->d, n, m->n_cu, m->ly.vw_chunks), dv, ds, nullptr, nullptr);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_score_views(dspmap_t* m, int n, const dspmap_view* views, int max_age, int flags, dspmap_view_score* out) {
    int rc = view_check(m, n, views, max_age, flags, out, "dspmap_score_views");
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    StageSec s[2] = {{views, nullptr, sizeof(dspmap_view) * (size_t)n}, {nullptr, out, sizeof(dspmap_view_score) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = view_score_enqueue(m, a, n, (const dspmap_view*)s[0].dev, (dspmap_view_score*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_score_views_device(dspmap_t* m, int n, const dspmap_view* views, int max_age, int flags, dspmap_view_score* out) {
    int rc = view_check(m, n, views, max_age, flags, out, "dspmap_score_views");
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    return view_score_enqueue(m, a, n, views, out);
}
extern "C" int dspmap_view_rays(dspmap_t* m, const float quat[4], float* planes_h, float* planes_v, float* dirs) {
    if (!m) return DSPMAP_E_ARG;
    if (!quat) return dspmap_fail(m, DSPMAP_E_ARG, "dspmap_view_rays: NULL quaternion");
    int rc = known_whole_map(m, "dspmap_view_rays");
    if (rc != DSPMAP_OK) return rc;
    READY(m);
    BENIGN(m);
    if ((rc = view_dirs(m)) != DSPMAP_OK) return rc;
    const MapDims& d = m->d;
    const size_t nh = 3 * (size_t)(d.np_h + 1), nv = 3 * (size_t)(d.np_v + 1), nd = 3 * (size_t)d.np;
    if ((rc = query_buf(m, sizeof(float) * (nh + nv + nd))) != DSPMAP_OK) return rc;
    ViewArgs a = {};
    view_args_geometry(m, &a, 0);
    float* o = (float*)m->ly.q_buf;
    launch_view_rays(d, m->s, m->stream, a, quat, o);
    HIPCHK(m, hipGetLastError());
    if (planes_h) HIPCHK(m, hipMemcpyAsync(planes_h, o, sizeof(float) * nh, hipMemcpyDeviceToHost, m->stream));
    if (planes_v) HIPCHK(m, hipMemcpyAsync(planes_v, o + nh, sizeof(float) * nv, hipMemcpyDeviceToHost, m->stream));
    if (dirs) HIPCHK(m, hipMemcpyAsync(dirs, o + nh + nv, sizeof(float) * nd, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return DSPMAP_OK;
}
// test hook: the seen set of ONE view as a bit grid in the cast grid's word layout, and the farthest returns its rays gave
extern "C" int dspmap_debug_view_cells(dspmap_t* m, const dspmap_view* view, int flags, unsigned long long* words_out, float* ml_out) {
    int rc = view_check(m, 1, view, 0, flags, words_out, "dspmap_debug_view_cells");
    if (rc != DSPMAP_OK) return rc;
    ViewArgs a;
    if ((rc = view_args(m, 0, flags, &a)) != DSPMAP_OK) return rc;
    const size_t lw = grid_layer_words(m->d);
    StageSec s[4] = {{view, nullptr, sizeof(dspmap_view)}, {nullptr, nullptr, sizeof(dspmap_view_score)}, {nullptr, words_out, sizeof(u64) * lw},
                     {nullptr, ml_out, sizeof(float) * (size_t)m->d.np}};
    if ((rc = stage_begin(m, s, 4)) != DSPMAP_OK) return rc;
    HIPCHK(m, hipMemsetAsync(s[1].dev, 0, (char*)s[3].dev - (char*)s[1].dev, m->stream));   // the score and the words: adjacent sections
    launch_view_score(m->d, m->s, m->stream, a, 1, view_chunks(m->d, 1, m->n_cu, m->ly.vw_chunks), (const dspmap_view*)s[0].dev,
                      (dspmap_view_score*)s[1].dev, (u64*)s[2].dev, (float*)s[3].dev);
    HIPCHK(m, hipGetLastError());
    return stage_end(m, s, 4);
}

// --------------------------------------------------- joint gain of views (dspmap_viewsel.hip; semantics in include/dspmap.h)
// what both calls check behind their own counts, in view_check's order: max_age, flags, the byte cap of the masks; then the state
static int view_sel_check(dspmap* m, const char* what, long long n, int max_age, int flags) {
    if (max_age < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative max_age %d", what, max_age);
    int rc = flags_check(m, what, flags, DSPMAP_QUERY_WORLD);
    if (rc != DSPMAP_OK) return rc;
    const unsigned long long mask = (unsigned long long)grid_layer_words(m->d) * sizeof(u64);   // (> 0)
    if ((unsigned long long)n > DSPMAP_VIEW_MASK_MAX_BYTES / mask)   // (a division: n * mask is formed only where it is known to be small)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: the masks of %lld views take %llu bytes, more than DSPMAP_VIEW_MASK_MAX_BYTES = %llu", what, n,
                           (unsigned long long)n > ~0ull / mask ? ~0ull : (unsigned long long)n * mask, (unsigned long long)DSPMAP_VIEW_MASK_MAX_BYTES);
    if ((rc = whole_map_check(m, what, "a view crosses slabs")) != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, what)) != DSPMAP_OK) return rc;
    if (!m->ly.kn_stamp || !m->ly.kn_integrated)
        return dspmap_fail(m, DSPMAP_E_STATE, "%s: no frame has been integrated into the known-space layer (dspmap_known_integrate)", what);
    return DSPMAP_OK;
}
static int view_sets_check(dspmap* m, int n_sets, int set_size, const void* views, int max_age, int flags, const void* out) {
    const char* what = "dspmap_score_view_sets";
    if (!m) return DSPMAP_E_ARG;
    if (n_sets < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative set count %d", what, n_sets);
    if (n_sets > 0 && (!views || !out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL view or output array", what);
    if (n_sets > 0 && set_size < 1) return dspmap_fail(m, DSPMAP_E_ARG, "%s: %d views per set", what, set_size);
    const long long n = (long long)n_sets * (n_sets > 0 ? set_size : 0);
    if (n > 0x7fffffffll) return dspmap_fail(m, DSPMAP_E_ARG, "%s: %d x %d views exceed INT_MAX", what, n_sets, set_size);
    return view_sel_check(m, what, n, max_age, flags);
}
static int view_select_check(dspmap* m, int n, const void* views, int n_fixed, int max_age, int flags, int k, int min_gain, const void* picks) {
    const char* what = "dspmap_select_views";
    if (!m) return DSPMAP_E_ARG;
    if (n < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative view count %d", what, n);
    if ((n > 0 && !views) || (k > 0 && !picks)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL view or pick array", what);
    if (n_fixed < 0 || n_fixed > n) return dspmap_fail(m, DSPMAP_E_ARG, "%s: n_fixed %d outside [0, %d]", what, n_fixed, n);
    if (k < 0 || k > DSPMAP_VIEW_MAX_PICKS) return dspmap_fail(m, DSPMAP_E_ARG, "%s: k %d outside [0, %d]", what, k, DSPMAP_VIEW_MAX_PICKS);
    if (min_gain < 1) return dspmap_fail(m, DSPMAP_E_ARG, "%s: min_gain %d below 1", what, min_gain);
    return view_sel_check(m, what, n, max_age, flags);
}
// the scratch of a call with n views: the masks, and behind them in one allocation (256-byte aligned sections, in this order)
struct ViewSelScratch { u64* masks; u64* unk; u64* avail; dspmap_view_set_score* fixed; dspmap_view_score* scores; int* gain; };
static int view_sel_scratch(dspmap* m, int n, ViewSelScratch* s) {
    LayerState& l = m->ly;
    const size_t lw = grid_layer_words(m->d);
    const size_t words = (size_t)n * lw;
    const size_t o_avail = q_align(sizeof(u64) * lw), o_fixed = o_avail + q_align(sizeof(u64) * lw), o_scores = o_fixed + q_align(sizeof(dspmap_view_set_score));
    const size_t o_gain = o_scores + q_align(sizeof(dspmap_view_score) * (size_t)n), bytes = o_gain + q_align(sizeof(int) * (size_t)n + sizeof(int));
    if (words > l.vs_masks_words || bytes > l.vs_aux_bytes) HIPCHK(m, hipStreamSynchronize(m->stream));   // (an earlier call may still use them)
    // (half as much again, as query_buf: a batch that creeps up does not drain the stream every time; the masks never beyond their cap)
    if (words > l.vs_masks_words) {
        if (l.vs_masks) { HIPCHK(m, hipFree(l.vs_masks)); l.vs_masks = nullptr; l.vs_masks_words = 0; }
        const size_t most = (size_t)(DSPMAP_VIEW_MASK_MAX_BYTES / sizeof(u64));
        size_t cap = words + words / 2;
        if (cap > most) cap = most;   // (words <= most: view_sel_check)
        HIPCHK(m, hipMalloc(&l.vs_masks, sizeof(u64) * cap));
        l.vs_masks_words = cap;
    }
    if (bytes > l.vs_aux_bytes) {
        if (l.vs_aux) { HIPCHK(m, hipFree(l.vs_aux)); l.vs_aux = nullptr; l.vs_aux_bytes = 0; }
        const size_t cap = bytes + bytes / 2;
        HIPCHK(m, hipMalloc(&l.vs_aux, cap));
        l.vs_aux_bytes = cap;
    }
    s->masks = l.vs_masks;
    s->unk = (u64*)l.vs_aux; s->avail = (u64*)(l.vs_aux + o_avail);
    s->fixed = (dspmap_view_set_score*)(l.vs_aux + o_fixed);
    s->scores = (dspmap_view_score*)(l.vs_aux + o_scores);
    s->gain = (int*)(l.vs_aux + o_gain);
    return DSPMAP_OK;
}
// the masks and scores of n views and UNK.  ds: the caller's scores [n], or NULL for the scratch's; *scores: where they are.  The masks
// are cleared first: k_view_score stores the non-zero words only (dspmap_view.hip says why)
static int view_masks_enqueue(dspmap* m, const ViewArgs& a, int n, const dspmap_view* dv, dspmap_view_score* ds, ViewSelScratch* s,
                              dspmap_view_score** scores) {
    const int rc = view_sel_scratch(m, n, s);
    if (rc != DSPMAP_OK) return rc;
    *scores = ds ? ds : s->scores;
    if (n > 0) {
        HIPCHK(m, hipMemsetAsync(s->masks, 0, sizeof(u64) * (size_t)n * grid_layer_words(m->d), m->stream));
        HIPCHK(m, hipMemsetAsync(*scores, 0, sizeof(dspmap_view_score) * (size_t)n, m->stream));
        launch_view_masks(m->d, m->s, m->stream, a, n, view_chunks(m->d, n, m->n_cu, m->ly.vw_chunks), dv, *scores, s->masks);
    }
    launch_viewsel_unknown(m->d, m->stream, a.kn, a.max_age, s->unk);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
// (the caller has filled the arguments, as for view_score_enqueue)
static int view_sets_enqueue(dspmap* m, const ViewArgs& a, int n_sets, int set_size, const dspmap_view* dv, dspmap_view_set_score* dout,
                             dspmap_view_score* ds) {
    ViewSelScratch s;
    dspmap_view_score* scores;
    const int rc = view_masks_enqueue(m, a, n_sets * set_size, dv, ds, &s, &scores);
    if (rc != DSPMAP_OK) return rc;
    const int lw = (int)grid_layer_words(m->d);
    HIPCHK(m, hipMemsetAsync(dout, 0, sizeof(dspmap_view_set_score) * (size_t)n_sets, m->stream));
    launch_viewsel_sets(m->stream, lw, n_sets, set_size, viewsel_chunks(lw, n_sets, m->n_cu, m->ly.vw_chunks), s.masks, s.unk, scores, dout, nullptr);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
// all k rounds are enqueued, whatever they pick: nothing is read back between them
static int view_select_enqueue(dspmap* m, const ViewArgs& a, int n, const dspmap_view* dv, int n_fixed, int k, int min_gain, dspmap_view_pick* dp,
                               dspmap_view_score* ds) {
    ViewSelScratch s;
    dspmap_view_score* scores;
    const int rc = view_masks_enqueue(m, a, n, dv, ds, &s, &scores);
    if (rc != DSPMAP_OK) return rc;
    if (k == 0) return DSPMAP_OK;
    const int lw = (int)grid_layer_words(m->d), n_cand = n - n_fixed;
    HIPCHK(m, hipMemsetAsync(s.fixed, 0, sizeof(dspmap_view_set_score), m->stream));
    HIPCHK(m, hipMemsetAsync(s.gain, 0, sizeof(int) * (size_t)n_cand + sizeof(int), m->stream));
    launch_viewsel_sets(m->stream, lw, 1, n_fixed, viewsel_chunks(lw, 1, m->n_cu, m->ly.vw_chunks), s.masks, s.unk, scores, s.fixed, s.avail);
    const int chunks = viewsel_chunks(lw, n_cand, m->n_cu, m->ly.vw_chunks);
    for (int r = 0; r < k; ++r) launch_viewsel_round(m->stream, lw, n_fixed, n_cand, chunks, r, min_gain, s.masks, s.avail, s.gain, s.fixed, dp);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_score_view_sets(dspmap_t* m, int n_sets, int set_size, const dspmap_view* views, int max_age, int flags,
                                      dspmap_view_set_score* out, dspmap_view_score* scores_out) {
    int rc = view_sets_check(m, n_sets, set_size, views, max_age, flags, out);
    if (rc != DSPMAP_OK) return rc;
    if (n_sets == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    const size_t n = (size_t)n_sets * set_size;
    StageSec s[3] = {{views, nullptr, sizeof(dspmap_view) * n}, {nullptr, out, sizeof(dspmap_view_set_score) * (size_t)n_sets},
                     {nullptr, scores_out, scores_out ? sizeof(dspmap_view_score) * n : 0}};   // (no scores asked for: the scratch holds them)
    if ((rc = stage_begin(m, s, 3)) != DSPMAP_OK) return rc;
    if ((rc = view_sets_enqueue(m, a, n_sets, set_size, (const dspmap_view*)s[0].dev, (dspmap_view_set_score*)s[1].dev, (dspmap_view_score*)s[2].dev)) != DSPMAP_OK)
        return rc;
    return stage_end(m, s, 3);
}
extern "C" int dspmap_score_view_sets_device(dspmap_t* m, int n_sets, int set_size, const dspmap_view* views, int max_age, int flags,
                                             dspmap_view_set_score* out, dspmap_view_score* scores_out) {
    int rc = view_sets_check(m, n_sets, set_size, views, max_age, flags, out);
    if (rc != DSPMAP_OK) return rc;
    if (n_sets == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    return view_sets_enqueue(m, a, n_sets, set_size, views, out, scores_out);
}
extern "C" int dspmap_select_views(dspmap_t* m, int n, const dspmap_view* views, int n_fixed, int max_age, int flags, int k, int min_gain,
                                   dspmap_view_pick* picks_out, dspmap_view_score* scores_out) {
    int rc = view_select_check(m, n, views, n_fixed, max_age, flags, k, min_gain, picks_out);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0 && k == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    StageSec s[3] = {{views, nullptr, sizeof(dspmap_view) * (size_t)n}, {nullptr, picks_out, sizeof(dspmap_view_pick) * (size_t)k},
                     {nullptr, scores_out, scores_out ? sizeof(dspmap_view_score) * (size_t)n : 0}};
    if ((rc = stage_begin(m, s, 3)) != DSPMAP_OK) return rc;
    if ((rc = view_select_enqueue(m, a, n, (const dspmap_view*)s[0].dev, n_fixed, k, min_gain, (dspmap_view_pick*)s[1].dev, (dspmap_view_score*)s[2].dev)) != DSPMAP_OK)
        return rc;
    return stage_end(m, s, 3);
}
extern "C" int dspmap_select_views_device(dspmap_t* m, int n, const dspmap_view* views, int n_fixed, int max_age, int flags, int k, int min_gain,
                                          dspmap_view_pick* picks_out, dspmap_view_score* scores_out) {
    int rc = view_select_check(m, n, views, n_fixed, max_age, flags, k, min_gain, picks_out);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0 && k == 0) return DSPMAP_OK;
    ViewArgs a;
    if ((rc = view_args(m, max_age, flags, &a)) != DSPMAP_OK) return rc;
    return view_select_enqueue(m, a, n, views, n_fixed, k, min_gain, picks_out, scores_out);
}

// --------------------------------------------------- frontier cells and blocks (dspmap_frontier.hip; semantics in include/dspmap.h)
// the layer t selects: the host twin of q_horizon (dspmap_device.h) + 1.  (t is not NaN here.)
static int frontier_layer_host(const MapDims& d, float t) {
    if (!(t >= 0.f) || d.T == 0) return 0;
    int k = d.T - 1;
    for (int j = d.T - 1; j >= 0; --j)
        if (d.pred_t[j] >= t) k = j;
    return k + 1;
}
// the buffers of a build with nb blocks: what does not depend on the block size once, the rest again when nb outgrows it
static int frontier_alloc(dspmap* m, size_t nb) {
    const MapDims& d = m->d;
    const size_t lw = grid_layer_words(d);
    if (!m->ly.fr_grid) HIPCHK(m, hipMalloc(&m->ly.fr_grid, sizeof(u64) * lw));
    if (!m->ly.fr_cells) HIPCHK(m, hipMalloc(&m->ly.fr_cells, sizeof(int) * (size_t)d.v_glob));
    if (!m->ly.fr_counts) HIPCHK(m, hipMalloc(&m->ly.fr_counts, 3 * sizeof(long long)));
    if (!m->ly.fr_item_free) HIPCHK(m, hipMalloc(&m->ly.fr_item_free, sizeof(int) * lw));
    if (nb > m->ly.fr_nb_cap) {
        if (m->ly.fr_nb_cap) HIPCHK(m, hipStreamSynchronize(m->stream));   // (an earlier build may still write the smaller buffers)
        for (void* q : {(void*)m->ly.fr_dense, (void*)m->ly.fr_blocks, (void*)m->ly.fr_tiles}) if (q) (void)hipFree(q);
        m->ly.fr_dense = nullptr; m->ly.fr_blocks = nullptr; m->ly.fr_tiles = nullptr; m->ly.fr_nb_cap = 0;
        HIPCHK(m, hipMalloc(&m->ly.fr_dense, sizeof(dspmap_frontier_block) * nb));
        HIPCHK(m, hipMalloc(&m->ly.fr_blocks, sizeof(dspmap_frontier_block) * nb));
        HIPCHK(m, hipMalloc(&m->ly.fr_tiles, sizeof(int) * (2 * (size_t)frontier_tiles((long long)lw) + (size_t)frontier_tiles((long long)nb))));
        m->ly.fr_nb_cap = nb;
    }
    return DSPMAP_OK;
}
extern "C" int dspmap_build_frontiers(dspmap_t* m, float t, int max_age, int min_unknown, int block, int flags) {
    const char* what = "dspmap_build_frontiers";
    if (!m) return DSPMAP_E_ARG;
    if (t != t) return dspmap_fail(m, DSPMAP_E_ARG, "%s: t is NaN", what);
    if (max_age < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative max_age %d", what, max_age);
    if (min_unknown < 1 || min_unknown > 6) return dspmap_fail(m, DSPMAP_E_ARG, "%s: min_unknown %d outside [1, 6]", what, min_unknown);
    if (block < 1 || block > DSPMAP_FRONTIER_MAX_BLOCK)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: block %d outside [1, %d]", what, block, DSPMAP_FRONTIER_MAX_BLOCK);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: unknown flags 0x%x", what, flags);
    int rc = whole_map_check(m, what, "a frontier crosses slabs");
    if (rc != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, what)) != DSPMAP_OK) return rc;
    if (!m->ly.kn_stamp || !m->ly.kn_integrated)
        return dspmap_fail(m, DSPMAP_E_STATE, "%s: no frame has been integrated into the known-space layer (dspmap_known_integrate)", what);
    const MapDims& d = m->d;
    dspmap_layers_stale(m->ly, LAYERS_FRONTIERS_REBUILD);
    FrontierArgs a;
    if ((rc = known_sync(m, &a.kn)) != DSPMAP_OK) return rc;
    a.nbx = (d.nx + block - 1) / block; a.nby = (d.ny + block - 1) / block;
    const size_t nb = (size_t)a.nbx * a.nby * (size_t)((d.nz + block - 1) / block);   // (<= V < 2^31)
    a.nb = (int)nb;
    if ((rc = frontier_alloc(m, nb)) != DSPMAP_OK) return rc;
    const size_t lw = grid_layer_words(d);
    a.bits = m->ly.cg_bits + lw * (size_t)frontier_layer_host(d, t);
    a.max_age = max_age; a.min_unknown = min_unknown; a.block = block;
    a.grid = m->ly.fr_grid; a.cells = m->ly.fr_cells; a.dense = m->ly.fr_dense; a.blocks = m->ly.fr_blocks;
    a.item_free = m->ly.fr_item_free;
    a.tile_sum = m->ly.fr_tiles;
    a.tile_free = m->ly.fr_tiles + frontier_tiles((long long)lw) + frontier_tiles((long long)nb);
    a.counts = m->ly.fr_counts;
    a.merge = m->ly.fr_merge ? 1 : 0;
    HIPCHK(m, hipMemsetAsync(m->ly.fr_dense, 0, sizeof(dspmap_frontier_block) * nb, m->stream));
    launch_frontiers(d, m->stream, a);
    HIPCHK(m, hipGetLastError());
    m->ly.fr_valid = true;
    return DSPMAP_OK;
}
static int frontier_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.fr_valid, what,
                          "no frontiers, or the grid, the known-space layer or the position has changed since they were built (dspmap_build_frontiers)");
}
extern "C" int dspmap_frontier_counts(dspmap_t* m, long long out[3]) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "dspmap_frontier_counts: NULL output array");
    const int rc = frontier_ready(m, "dspmap_frontier_counts");
    if (rc != DSPMAP_OK) return rc;
    return read_back(m, out, m->ly.fr_counts, 3 * sizeof(long long));
}
extern "C" int dspmap_get_frontier_grid(dspmap_t* m, unsigned long long* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "dspmap_get_frontier_grid: NULL output array");
    const int rc = frontier_ready(m, "dspmap_get_frontier_grid");
    if (rc != DSPMAP_OK) return rc;
    return read_back(m, out, m->ly.fr_grid, sizeof(u64) * grid_layer_words(m->d));
}
// the first min(cap, n) entries of list `which` (0: cells, 1: blocks) of `bytes` each, and n
static int frontier_list(dspmap* m, const char* what, int which, const void* dev, size_t bytes, int cap, void* out, int* n_out) {
    if (!m) return DSPMAP_E_ARG;
    if (cap < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative capacity %d", what, cap);
    if (!n_out || (cap > 0 && !out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL output", what);
    int rc = frontier_ready(m, what);
    if (rc != DSPMAP_OK) return rc;
    long long c[3];
    if ((rc = read_back(m, c, m->ly.fr_counts, sizeof(c))) != DSPMAP_OK) return rc;
    const long long n = c[which], take = n < cap ? n : cap;
    if (take > 0 && (rc = read_back(m, out, dev, bytes * (size_t)take)) != DSPMAP_OK) return rc;
    *n_out = (int)n;
    return DSPMAP_OK;
}
extern "C" int dspmap_get_frontier_cells(dspmap_t* m, int cap, int* out, int* n_out) {
    return frontier_list(m, "dspmap_get_frontier_cells", 0, m ? m->ly.fr_cells : nullptr, sizeof(int), cap, out, n_out);
}
extern "C" int dspmap_get_frontier_blocks(dspmap_t* m, int cap, dspmap_frontier_block* out, int* n_out) {
    return frontier_list(m, "dspmap_get_frontier_blocks", 1, m ? m->ly.fr_blocks : nullptr, sizeof(dspmap_frontier_block), cap, out, n_out);
}
extern "C" const unsigned long long* dspmap_frontier_grid_device(dspmap_t* m) { return (m && m->ly.fr_valid) ? m->ly.fr_grid : nullptr; }
extern "C" const int* dspmap_frontier_cells_device(dspmap_t* m) { return (m && m->ly.fr_valid) ? m->ly.fr_cells : nullptr; }
extern "C" const dspmap_frontier_block* dspmap_frontier_blocks_device(dspmap_t* m) { return (m && m->ly.fr_valid) ? m->ly.fr_blocks : nullptr; }
extern "C" const long long* dspmap_frontier_counts_device(dspmap_t* m) { return (m && m->ly.fr_valid) ? m->ly.fr_counts : nullptr; }
// test hook: the ages of the known-space layer replaced cell by cell, written through the toroidal slot mapping
extern "C" int dspmap_debug_set_known(dspmap_t* m, const int* age) {
    if (!m) return DSPMAP_E_ARG;
    if (!age) return dspmap_fail(m, DSPMAP_E_ARG, "set known: NULL age array");
    int rc = known_whole_map(m, "dspmap_debug_set_known");
    if (rc != DSPMAP_OK) return rc;
    if (m->update_counter < 1)
        return dspmap_fail(m, DSPMAP_E_STATE, "set known: no frame has been accepted yet, there is no counter to age against (dspmap_update)");
    const MapDims& d = m->d;
    const size_t V = (size_t)d.v_glob;
    for (size_t i = 0; i < V; ++i)
        if (age[i] < -1 || age[i] > m->update_counter - 1)
            return dspmap_fail(m, DSPMAP_E_ARG, "set known: age[%zu] = %d outside [-1, %d]", i, age[i], m->update_counter - 1);
    READY(m);
    BENIGN(m);
    dspmap_layers_stale(m->ly, LAYERS_KNOWN_CHANGED);
    if (!m->ly.kn_stamp) {
        HIPCHK(m, hipMalloc(&m->ly.kn_stamp, sizeof(unsigned) * V));
        HIPCHK(m, hipMemsetAsync(m->ly.kn_stamp, 0, sizeof(unsigned) * V, m->stream));
    }
    KnownArgs a;
    if ((rc = known_sync(m, &a)) != DSPMAP_OK) return rc;
    std::vector<unsigned> stamp(V);
    auto slot = [](int i, int b, int n) { const int s = i + b; return s >= n ? s - n : s; };   // kn_slot
    size_t g = 0;
    for (int z = 0; z < d.nz; ++z)
        for (int y = 0; y < d.ny; ++y) {
            unsigned* row = &stamp[((size_t)slot(z, a.bz, d.nz) * d.ny + slot(y, a.by, d.ny)) * d.nx];
            for (int x = 0; x < d.nx; ++x, ++g) row[slot(x, a.bx, d.nx)] = age[g] < 0 ? 0u : a.now - (unsigned)age[g];
        }
    HIPCHK(m, hipMemcpyAsync(m->ly.kn_stamp, stamp.data(), sizeof(unsigned) * V, hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));   // (the local array is free again)
    m->ly.kn_integrated = true;
    return DSPMAP_OK;
}

// --------------------------------------------------- objects: components of a cast-grid layer (dspmap_objects.hip; semantics in include/dspmap.h)
#define DSPMAP_OBJECTS_MAX (1 << 20)
// the buffers of a build that keeps `cap` records: what depends on V alone once, the records again when cap outgrows them
static int objects_alloc(dspmap* m, size_t cap) {
    const size_t V = (size_t)m->d.v_glob;
    if (!m->ly.ob_parent) HIPCHK(m, hipMalloc(&m->ly.ob_parent, sizeof(int) * V));
    if (!m->ly.ob_root) HIPCHK(m, hipMalloc(&m->ly.ob_root, sizeof(int) * V));
    if (!m->ly.ob_labels) HIPCHK(m, hipMalloc(&m->ly.ob_labels, sizeof(int) * V));
    if (!m->ly.ob_tiles) HIPCHK(m, hipMalloc(&m->ly.ob_tiles, sizeof(int) * (size_t)frontier_tiles((long long)V)));
    if (!m->ly.ob_counts) HIPCHK(m, hipMalloc(&m->ly.ob_counts, OBJ_COUNTS * sizeof(long long)));
    if (cap > m->ly.ob_cap) {
        if (m->ly.ob_cap) HIPCHK(m, hipStreamSynchronize(m->stream));   // (an earlier build may still write the smaller buffer)
        if (m->ly.ob_objects) { (void)hipFree(m->ly.ob_objects); m->ly.ob_objects = nullptr; m->ly.ob_cap = 0; }
        HIPCHK(m, hipMalloc(&m->ly.ob_objects, sizeof(dspmap_object) * cap));
        m->ly.ob_cap = cap;
    }
    return DSPMAP_OK;
}
extern "C" int dspmap_build_objects(dspmap_t* m, float t, int connectivity, int min_cells, int max_objects, int flags) {
    const char* what = "dspmap_build_objects";
    if (!m) return DSPMAP_E_ARG;
    if (t != t) return dspmap_fail(m, DSPMAP_E_ARG, "%s: t is NaN", what);
    if (connectivity != 6 && connectivity != 26) return dspmap_fail(m, DSPMAP_E_ARG, "%s: connectivity %d is neither 6 nor 26", what, connectivity);
    if (min_cells < 1) return dspmap_fail(m, DSPMAP_E_ARG, "%s: min_cells %d below 1", what, min_cells);
    if (max_objects < 1 || max_objects > DSPMAP_OBJECTS_MAX)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: max_objects %d outside [1, %d]", what, max_objects, DSPMAP_OBJECTS_MAX);
    if (flags != 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: unknown flags 0x%x", what, flags);
    int rc = whole_map_check(m, what, "components cross slabs");
    if (rc != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, what)) != DSPMAP_OK) return rc;
    const MapDims& d = m->d;
    const size_t V = (size_t)d.v_glob;
    dspmap_layers_stale(m->ly, LAYERS_OBJECTS_REBUILD);
    if ((rc = objects_alloc(m, (size_t)max_objects < V ? (size_t)max_objects : V)) != DSPMAP_OK) return rc;
    ObjectArgs a;
    a.bits = m->ly.cg_bits + grid_layer_words(d) * (size_t)frontier_layer_host(d, t);
    a.conn = connectivity; a.min_cells = min_cells; a.max_objects = max_objects;
    a.parent = m->ly.ob_parent; a.root_val = m->ly.ob_root; a.labels = m->ly.ob_labels; a.objects = m->ly.ob_objects;
    a.tile_sum = m->ly.ob_tiles; a.counts = m->ly.ob_counts;
    HIPCHK(m, hipMemsetAsync(m->ly.ob_root, 0, sizeof(int) * V, m->stream));
    HIPCHK(m, hipMemsetAsync(m->ly.ob_counts, 0, OBJ_COUNTS * sizeof(long long), m->stream));
    launch_objects(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    m->ly.ob_max = max_objects;
    m->ly.ob_valid = true;
    return DSPMAP_OK;
}
static int objects_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.ob_valid, what, "no objects, or the map or its cast grid has changed since they were built (dspmap_build_objects)");
}
// the counts of the valid build, read back; a non-zero fault word (the labelling met a broken invariant or ran out of a trip bound) is an error
static int objects_counts(dspmap* m, const char* what, long long c[OBJ_COUNTS]) {
    const int rc = read_back(m, c, m->ly.ob_counts, OBJ_COUNTS * sizeof(long long));
    if (rc != DSPMAP_OK) return rc;
    if (c[3] != 0) return dspmap_fail(m, DSPMAP_E_DEVICE, "%s: the labelling of the last dspmap_build_objects gave up (fault word 0x%llx)", what, (unsigned long long)c[3]);
    return DSPMAP_OK;
}
extern "C" int dspmap_object_counts(dspmap_t* m, long long out[3]) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "dspmap_object_counts: NULL output array");
    int rc = objects_ready(m, "dspmap_object_counts");
    if (rc != DSPMAP_OK) return rc;
    long long c[OBJ_COUNTS];
    if ((rc = objects_counts(m, "dspmap_object_counts", c)) != DSPMAP_OK) return rc;
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    return DSPMAP_OK;
}
extern "C" int dspmap_get_objects(dspmap_t* m, int cap, dspmap_object* out, int* n_out) {
    const char* what = "dspmap_get_objects";
    if (!m) return DSPMAP_E_ARG;
    if (cap < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative capacity %d", what, cap);
    if (!n_out || (cap > 0 && !out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL output", what);
    int rc = objects_ready(m, what);
    if (rc != DSPMAP_OK) return rc;
    long long c[OBJ_COUNTS];
    if ((rc = objects_counts(m, what, c)) != DSPMAP_OK) return rc;
    const long long n = c[0] < m->ly.ob_max ? c[0] : m->ly.ob_max, take = n < cap ? n : cap;   // the records the build kept
    if (take > 0 && (rc = read_back(m, out, m->ly.ob_objects, sizeof(dspmap_object) * (size_t)take)) != DSPMAP_OK) return rc;
    *n_out = (int)n;
    return DSPMAP_OK;
}
extern "C" int dspmap_get_object_labels(dspmap_t* m, int* out) {
    const char* what = "dspmap_get_object_labels";
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL output array", what);
    int rc = objects_ready(m, what);
    if (rc != DSPMAP_OK) return rc;
    long long c[OBJ_COUNTS];
    if ((rc = objects_counts(m, what, c)) != DSPMAP_OK) return rc;
    return read_back(m, out, m->ly.ob_labels, sizeof(int) * (size_t)m->d.v_glob);
}
extern "C" const dspmap_object* dspmap_objects_device(dspmap_t* m) { return (m && m->ly.ob_valid) ? m->ly.ob_objects : nullptr; }
extern "C" const int* dspmap_object_labels_device(dspmap_t* m) { return (m && m->ly.ob_valid) ? m->ly.ob_labels : nullptr; }
extern "C" const long long* dspmap_object_counts_device(dspmap_t* m) { return (m && m->ly.ob_valid) ? m->ly.ob_counts : nullptr; }
static int objects_query_check(dspmap* m, int n, const void* in, const void* out, int flags) {
    if (!m) return DSPMAP_E_ARG;
    int rc = samples_check(m, "objects query", "sample", n, in, out);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = flags_check(m, "objects query", flags, DSPMAP_QUERY_WORLD)) != DSPMAP_OK) return rc;
    return objects_ready(m, "dspmap_query_objects");
}
static int objects_query_enqueue(dspmap* m, int n, const float4* dq, int flags, int* dout) {
    launch_objects_query(dspmap_ctx_of(m), m->ly.ob_labels, origin_fill(m, flags), n, dq, dout);
    HIPCHK(m, hipGetLastError());
    return DSPMAP_OK;
}
extern "C" int dspmap_query_objects(dspmap_t* m, int n, const dspmap_query* q, int flags, int* ordinal_out) {
    int rc = objects_query_check(m, n, q, ordinal_out, flags);
    if (rc != DSPMAP_OK) return rc;
    if (n == 0) return DSPMAP_OK;
    StageSec s[2] = {{q, nullptr, sizeof(dspmap_query) * (size_t)n}, {nullptr, ordinal_out, sizeof(int) * (size_t)n}};
    if ((rc = stage_begin(m, s, 2)) != DSPMAP_OK) return rc;
    if ((rc = objects_query_enqueue(m, n, (const float4*)s[0].dev, flags, (int*)s[1].dev)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 2);
}
extern "C" int dspmap_query_objects_device(dspmap_t* m, int n, const dspmap_query* q, int flags, int* ordinal_out) {
    const int rc = objects_query_check(m, n, q, ordinal_out, flags);
    if (rc != DSPMAP_OK) return rc;
    return objects_query_enqueue(m, n, (const float4*)q, flags, ordinal_out);
}

// --------------------------------------------------- tracks: objects across builds (dspmap_track.hip; semantics in include/dspmap.h)
static_assert(DSPMAP_OBJECTS_MAX <= (1 << TRK_ORD_BITS), "a pair's key holds two ordinals of TRK_ORD_BITS bits");
#define DSPMAP_TRACK_MAX_SHIFT 64
#define DSPMAP_TRACK_MAX_SLOTS (1 << 24)
// a per-record array of the tracker grown from `old_n` to `n` records of `bytes` each (the stream has drained); keep: with its contents
template <class T> static int track_grow(dspmap* m, T** p, size_t old_n, size_t n, bool keep) {
    T* q = nullptr;
    HIPCHK(m, hipMalloc(&q, sizeof(T) * n));
    if (keep && *p && old_n) HIPCHK(m, hipMemcpy(q, *p, sizeof(T) * old_n, hipMemcpyDeviceToDevice));
    if (*p) (void)hipFree(*p);
    *p = q;
    return DSPMAP_OK;
}
// the tracker's buffers for `cap` records and a table of `slots`: what depends on V alone once, the rest again when it is outgrown.  What
// an update clears -- the two best arrays [cap] and the table's keys and counts [slots] -- is ONE allocation, cleared by one memset
static size_t track_zero_bytes(size_t cap, size_t slots) { return 2 * sizeof(u64) * cap + (sizeof(u64) + sizeof(int)) * slots; }
static int track_alloc(dspmap* m, size_t cap, size_t slots) {
    LayerState& l = m->ly;
    int rc;
    if (!l.tk_labels) HIPCHK(m, hipMalloc(&l.tk_labels, sizeof(int) * (size_t)m->d.v_glob));
    if (!l.tk_counts) {
        HIPCHK(m, hipMalloc(&l.tk_counts, TRK_WORDS * sizeof(long long)));
        HIPCHK(m, hipMemsetAsync(l.tk_counts, 0, TRK_WORDS * sizeof(long long), m->stream));
    }
    if (cap > l.tk_cap) {
        if (l.tk_cap) HIPCHK(m, hipStreamSynchronize(m->stream));   // (an earlier update may still use the smaller arrays)
        const size_t old = l.tk_cap;
        const size_t tiles = (size_t)frontier_tiles((long long)cap), old_tiles = (size_t)frontier_tiles((long long)old);
        if ((rc = track_grow(m, &l.tk_objects, old, cap, true)) != DSPMAP_OK) return rc;
        if ((rc = track_grow(m, &l.tk_tracks[l.tk_cur], old, cap, true)) != DSPMAP_OK) return rc;
        if ((rc = track_grow(m, &l.tk_tracks[l.tk_cur ^ 1], old, cap, false)) != DSPMAP_OK) return rc;
        if ((rc = track_grow(m, &l.tk_shift, old, cap, false)) != DSPMAP_OK) return rc;
        if ((rc = track_grow(m, &l.tk_tiles, old_tiles, tiles, false)) != DSPMAP_OK) return rc;
        l.tk_cap = cap;
    }
    const size_t zero = track_zero_bytes(l.tk_cap, slots);
    if (zero > l.tk_zero_bytes) {
        if (l.tk_zero_bytes) HIPCHK(m, hipStreamSynchronize(m->stream));
        if ((rc = track_grow(m, &l.tk_zero, l.tk_zero_bytes, zero, false)) != DSPMAP_OK) return rc;
        l.tk_zero_bytes = zero;
    }
    return DSPMAP_OK;
}
// everything forgotten (dspmap_track_reset, dspmap_clear_state, dspmap_load_checkpoint); a handle that never tracked has nothing to forget
int dspmap_track_forget(dspmap* m) {
    LayerState& l = m->ly;
    l.tk_have = false; l.tk_valid = false; l.tk_seq = 0;
    if (l.tk_counts) {
        if (m->device >= 0) (void)hipSetDevice(m->device);
        HIPCHK(m, hipMemsetAsync(l.tk_counts, 0, TRK_WORDS * sizeof(long long), m->stream));
    }
    return DSPMAP_OK;
}
extern "C" int dspmap_track_reset(dspmap_t* m) {
    if (!m) return DSPMAP_E_ARG;
    return dspmap_track_forget(m);
}
extern "C" int dspmap_track_update(dspmap_t* m, float dt, int min_overlap, int max_shift, int max_pairs, int flags) {
    const char* what = "dspmap_track_update";
    if (!m) return DSPMAP_E_ARG;
    if (!(dt >= 0.f && dt < INFINITY)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: dt %g is NaN, negative or infinite", what, (double)dt);
    if (min_overlap < 1) return dspmap_fail(m, DSPMAP_E_ARG, "%s: min_overlap %d below 1", what, min_overlap);
    if (max_shift < 0 || max_shift > DSPMAP_TRACK_MAX_SHIFT)
        return dspmap_fail(m, DSPMAP_E_ARG, "%s: max_shift %d outside [0, %d]", what, max_shift, DSPMAP_TRACK_MAX_SHIFT);
    if (max_pairs < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative max_pairs %d", what, max_pairs);
    int rc = flags_check(m, what, flags, DSPMAP_TRACK_PER_CELL);
    if (rc != DSPMAP_OK) return rc;
    if ((rc = whole_map_check(m, what, "components cross slabs")) != DSPMAP_OK) return rc;
    if ((rc = objects_ready(m, what)) != DSPMAP_OK) return rc;
    long long k0[3];
    float o[3];
    if ((rc = known_window(m, k0, o)) != DSPMAP_OK) return rc;
    LayerState& l = m->ly;
    const MapDims& d = m->d;
    const size_t V = (size_t)d.v_glob;
    // the table: max_pairs (0: 8 x the record capacity, at least 1024) rounded up to a power of two, at most 2^24 slots
    size_t want = max_pairs > 0 ? (size_t)max_pairs : (8 * l.ob_cap > 1024 ? 8 * l.ob_cap : 1024), slots = 1;
    while (slots < want && slots < DSPMAP_TRACK_MAX_SLOTS) slots <<= 1;
    if ((rc = track_alloc(m, l.ob_cap, slots)) != DSPMAP_OK) return rc;
    TrackArgs a;
    a.fresh = l.tk_have ? 0 : 1;
    const int n[3] = {d.nx, d.ny, d.nz};
    for (int ax = 0; ax < 3; ++ax) {
        const long long delta = l.tk_have ? k0[ax] - l.tk_k0[ax] : 0;
        if (delta >= n[ax] || -delta >= n[ax]) a.fresh = 1;   // the window moved by a whole map: nothing of the previous grid is in it
        a.dk0[ax] = a.fresh ? 0 : (int)delta;
    }
    if (a.fresh) a.dk0[0] = a.dk0[1] = a.dk0[2] = 0;          // (a later axis may have decided)
    a.labels = l.ob_labels; a.objects = l.ob_objects; a.obj_counts = l.ob_counts; a.max_objects = l.ob_max;
    a.p_labels = l.tk_labels; a.p_objects = l.tk_objects; a.p_tracks = l.tk_tracks[l.tk_cur]; a.tracks = l.tk_tracks[l.tk_cur ^ 1];
    a.shift = l.tk_shift;
    a.best_prev = (u64*)l.tk_zero; a.best_now = a.best_prev + l.tk_cap; a.keys = a.best_now + l.tk_cap; a.vals = (int*)(a.keys + slots);
    a.slots = (int)slots; a.tile_sum = l.tk_tiles; a.counts = l.tk_counts; a.cap = (int)l.tk_cap;
    a.min_overlap = min_overlap; a.max_shift = max_shift; a.per_cell = (flags & DSPMAP_TRACK_PER_CELL) ? 1 : 0; a.seq = l.tk_seq; a.dt = dt;
    HIPCHK(m, hipMemsetAsync(l.tk_counts, 0, (TRK_FAULT + 1) * sizeof(long long), m->stream));
    if (!a.fresh) HIPCHK(m, hipMemsetAsync(l.tk_zero, 0, track_zero_bytes(l.tk_cap, slots), m->stream));
    launch_track(dspmap_ctx_of(m), a);
    HIPCHK(m, hipGetLastError());
    // what the next update associates with: this build's label grid and records (k_track_keep has set their number)
    const size_t kept = (size_t)l.ob_max < V ? (size_t)l.ob_max : V;   // (<= ob_cap <= tk_cap)
    HIPCHK(m, hipMemcpyAsync(l.tk_labels, l.ob_labels, sizeof(int) * V, hipMemcpyDeviceToDevice, m->stream));
    HIPCHK(m, hipMemcpyAsync(l.tk_objects, l.ob_objects, sizeof(dspmap_object) * kept, hipMemcpyDeviceToDevice, m->stream));
    l.tk_cur ^= 1;
    for (int ax = 0; ax < 3; ++ax) l.tk_k0[ax] = k0[ax];
    l.tk_have = true; l.tk_valid = true; l.tk_slots = (int)slots;
    ++l.tk_seq;
    return DSPMAP_OK;
}
static int tracks_ready(dspmap* m, const char* what) {
    return snapshot_ready(m, m->ly.tk_valid, what, "no tracks: no update since the handle was created, reset or given a new state (dspmap_track_update)");
}
// the counts of the last update, read back; a set fault word (the pair table was full, the update is void) is an error
static int tracks_counts(dspmap* m, const char* what, long long c[TRK_FAULT + 1]) {
    const int rc = read_back(m, c, m->ly.tk_counts, (TRK_FAULT + 1) * sizeof(long long));
    if (rc != DSPMAP_OK) return rc;
    if (c[TRK_FAULT] != 0)
        return dspmap_fail(m, DSPMAP_E_DEVICE, "%s: the pair table of the last dspmap_track_update was full (max_pairs: %d slots), the update is void", what,
                           m->ly.tk_slots);
    return DSPMAP_OK;
}
extern "C" int dspmap_track_counts(dspmap_t* m, long long out[6]) {
    const char* what = "dspmap_track_counts";
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL output array", what);
    int rc = tracks_ready(m, what);
    if (rc != DSPMAP_OK) return rc;
    long long c[TRK_FAULT + 1];
    if ((rc = tracks_counts(m, what, c)) != DSPMAP_OK) return rc;
    for (int i = 0; i < TRK_COUNTS; ++i) out[i] = c[i];
    return DSPMAP_OK;
}
extern "C" int dspmap_get_tracks(dspmap_t* m, int cap, dspmap_track* out, int* n_out) {
    const char* what = "dspmap_get_tracks";
    if (!m) return DSPMAP_E_ARG;
    if (cap < 0) return dspmap_fail(m, DSPMAP_E_ARG, "%s: negative capacity %d", what, cap);
    if (!n_out || (cap > 0 && !out)) return dspmap_fail(m, DSPMAP_E_ARG, "%s: NULL output", what);
    int rc = tracks_ready(m, what);
    if (rc != DSPMAP_OK) return rc;
    long long c[TRK_FAULT + 1];
    if ((rc = tracks_counts(m, what, c)) != DSPMAP_OK) return rc;
    const long long n = c[0], take = n < cap ? n : cap;
    if (take > 0 && (rc = read_back(m, out, m->ly.tk_tracks[m->ly.tk_cur], sizeof(dspmap_track) * (size_t)take)) != DSPMAP_OK) return rc;
    *n_out = (int)n;
    return DSPMAP_OK;
}
extern "C" const dspmap_track* dspmap_tracks_device(dspmap_t* m) { return (m && m->ly.tk_valid) ? m->ly.tk_tracks[m->ly.tk_cur] : nullptr; }
extern "C" const long long* dspmap_track_counts_device(dspmap_t* m) { return (m && m->ly.tk_valid) ? m->ly.tk_counts : nullptr; }

// --------------------------------------------------- cost-to-go fields (dspmap_cost.hip; semantics in include/dspmap.h)
static_assert(COST_MAX_BANDS == DSPMAP_COST_MAX_BANDS && COST_MAX_WEIGHT == DSPMAP_COST_MAX_WEIGHT, "CostWeightArgs holds DSPMAP_COST_MAX_BANDS bands");
static_assert(sizeof(dspmap_cost_bands) == 36, "dspmap_cost_bands is 36 bytes");
// the checks of both builds, in the header's order: arguments, then slab, cast grid and (with bands) distance field
static int cost_build_check(dspmap* m, int n_fields, int n_src, const void* src, float t, const dspmap_cost_bands* bands, int max_cost, int flags) {
    if (!m) return DSPMAP_E_ARG;
    if (n_fields < 1 || n_fields > DSPMAP_COST_MAX_FIELDS)
        return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: n_fields %d outside [1, %d]", n_fields, DSPMAP_COST_MAX_FIELDS);
    if (n_src < 0) return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: negative source count %d", n_src);
    if (n_src > 0 && !src) return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: NULL source array");
    if (t != t) return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: t is NaN");
    if (!bands) return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: NULL bands");
    if (bands->n_bands < 0 || bands->n_bands > DSPMAP_COST_MAX_BANDS)
        return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: n_bands %d outside [0, %d]", bands->n_bands, DSPMAP_COST_MAX_BANDS);
    for (int i = 0; i < bands->n_bands; ++i)
        if (!(bands->clearance[i] > 0.f && bands->clearance[i] < INFINITY))
            return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: clearance[%d] = %g is NaN, infinite or not positive", i, (double)bands->clearance[i]);
    int total = 1;
    for (int i = 0; i < bands->n_bands; ++i) {
        if (bands->penalty[i] < 0 || bands->penalty[i] > DSPMAP_COST_MAX_WEIGHT - 1)
            return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: penalty[%d] = %d outside [0, %d]", i, bands->penalty[i], DSPMAP_COST_MAX_WEIGHT - 1);
        total += bands->penalty[i];
    }
    if (total > DSPMAP_COST_MAX_WEIGHT)
        return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: the largest weight 1 + sum of penalty = %d exceeds DSPMAP_COST_MAX_WEIGHT = %d", total,
                           DSPMAP_COST_MAX_WEIGHT);
    if (max_cost < 1 || max_cost > DSPMAP_COST_MAX_COST)
        return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: max_cost %d outside [1, %d]", max_cost, DSPMAP_COST_MAX_COST);
    int rc = flags_check(m, "cost fields", flags, DSPMAP_QUERY_WORLD);
    if (rc != DSPMAP_OK) return rc;
    const unsigned long long cells = (unsigned long long)n_fields * (unsigned long long)m->d.v_glob;
    if (cells > 0x80000000ull) return dspmap_fail(m, DSPMAP_E_ARG, "cost fields: %d fields of %d cells exceed 2^31 cells", n_fields, m->d.v_glob);
    if ((rc = whole_map_check(m, "cost fields", "a wavefront crosses slabs")) != DSPMAP_OK) return rc;
    if ((rc = cast_grid_ready(m, "dspmap_build_cost_fields")) != DSPMAP_OK) return rc;
    return bands->n_bands > 0 ? dist_field_ready(m, "dspmap_build_cost_fields") : DSPMAP_OK;
}
// the two launches behind both build entry points; src_dev may be NULL with n_src == 0
static int cost_build(dspmap* m, int n_fields, int n_src, const dspmap_reach_point* src_dev, float t, const dspmap_cost_bands* bands, int max_cost,
                      int flags) {
    const MapDims& d = m->d;
    dspmap_layers_stale(m->ly, LAYERS_COST_REBUILD);
    const size_t V = (size_t)d.v_glob, cells = (size_t)n_fields * V, lw = grid_layer_words(d);
    const size_t set_words = (size_t)COST_SET_COUNT * lw * (size_t)n_fields;
    if (!m->ly.cf_weight || cells > m->ly.cf_field_cells || set_words > m->ly.cf_sets_words) {   // grown only after the stream has drained (an earlier call may still read them)
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (!m->ly.cf_weight) HIPCHK(m, hipMalloc(&m->ly.cf_weight, V));
        if (!m->ly.cf_wk) HIPCHK(m, hipMalloc(&m->ly.cf_wk, sizeof(u64) * COST_MAX_WEIGHT * lw));
        if (!m->ly.cf_occ) HIPCHK(m, hipMalloc(&m->ly.cf_occ, sizeof(int)));
        int rc = layer_buf_grow(m, &m->ly.cf_field, &m->ly.cf_field_cells, cells);
        if (rc == DSPMAP_OK) rc = layer_buf_grow(m, &m->ly.cf_sets, &m->ly.cf_sets_words, set_words);
        if (rc != DSPMAP_OK) return rc;
    }
    const int l = frontier_layer_host(d, t);   // ONE layer for the whole build: dspmap_build_objects' rule
    CostWeightArgs w;
    w.n_bands = bands->n_bands;
    for (int i = 0; i < COST_MAX_BANDS; ++i) {
        w.clearance[i] = i < bands->n_bands ? bands->clearance[i] : 0.f;
        w.penalty[i] = i < bands->n_bands ? bands->penalty[i] : 0;
    }
    w.bits = m->ly.cg_bits + lw * (size_t)l;
    w.dist = bands->n_bands > 0 ? m->ly.df_field + V * (size_t)l : nullptr;
    w.weight = m->ly.cf_weight; w.wk = m->ly.cf_wk; w.occ = m->ly.cf_occ;
    CostArgs a;
    a.org = origin_fill(m, flags);
    a.max_cost = max_cost; a.n_fields = n_fields; a.n_src = n_src;
    a.wk = m->ly.cf_wk; a.occ = m->ly.cf_occ; a.field = m->ly.cf_field; a.sets = m->ly.cf_sets;
    const LaunchCtx c = dspmap_ctx_of(m);
    HIPCHK(m, hipMemsetAsync(m->ly.cf_occ, 0, sizeof(int), m->stream));
    launch_cost_weights(c, w);
    HIPCHK(m, hipMemsetAsync(m->ly.cf_field, 0xff, sizeof(unsigned short) * cells, m->stream));   // every value DSPMAP_COST_UNREACHED
    launch_cost_wave(c, a, src_dev);
    HIPCHK(m, hipGetLastError());
    m->ly.cf_n = n_fields;
    m->ly.cf_valid = true;
    return DSPMAP_OK;
}
extern "C" int dspmap_build_cost_fields(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t, const dspmap_cost_bands* bands,
                                        int max_cost, int flags) {
    int rc = cost_build_check(m, n_fields, n_src, src, t, bands, max_cost, flags);
    if (rc != DSPMAP_OK) return rc;
    StageSec s[1] = {{src, nullptr, sizeof(dspmap_reach_point) * (size_t)n_src}};   // (no sources: no section, the kernel gets NULL)
    if ((rc = stage_begin(m, s, 1)) != DSPMAP_OK) return rc;
    if ((rc = cost_build(m, n_fields, n_src, (const dspmap_reach_point*)s[0].dev, t, bands, max_cost, flags)) != DSPMAP_OK) return rc;
    return stage_end(m, s, 1);
}
extern "C" int dspmap_build_cost_fields_device(dspmap_t* m, int n_fields, int n_src, const dspmap_reach_point* src, float t,
                                               const dspmap_cost_bands* bands, int max_cost, int flags) {
    const int rc = cost_build_check(m, n_fields, n_src, src, t, bands, max_cost, flags);
    if (rc != DSPMAP_OK) return rc;
    return cost_build(m, n_fields, n_src, src, t, bands, max_cost, flags);
}
extern "C" const unsigned short* dspmap_cost_fields_device(dspmap_t* m) { return (m && m->ly.cf_valid) ? m->ly.cf_field : nullptr; }
extern "C" const unsigned char* dspmap_cost_weights_device(dspmap_t* m) { return (m && m->ly.cf_valid) ? m->ly.cf_weight : nullptr; }
static int cost_ready(dspmap* m, const char* what) {
    const int rc = whole_map_check(m, what, "a wavefront crosses slabs");
    if (rc != DSPMAP_OK) return rc;
    return snapshot_ready(m, m->ly.cf_valid, what,
                          "no cost fields, or the map, its cast grid or its distance field has changed since they were built (dspmap_build_cost_fields)");
}
extern "C" int dspmap_get_cost_field(dspmap_t* m, int field, unsigned short* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "cost field: NULL output array");
    if (field < 0 || field >= DSPMAP_COST_MAX_FIELDS) return dspmap_fail(m, DSPMAP_E_ARG, "cost field: field %d outside [0, %d)", field, DSPMAP_COST_MAX_FIELDS);
    const int rc = cost_ready(m, "dspmap_get_cost_field");
    if (rc != DSPMAP_OK) return rc;
    if (field >= m->ly.cf_n) return dspmap_fail(m, DSPMAP_E_ARG, "cost field: field %d outside [0, %d), the fields of the last build", field, m->ly.cf_n);
    return read_back(m, out, m->ly.cf_field + (size_t)field * m->d.v_glob, sizeof(unsigned short) * (size_t)m->d.v_glob);
}
extern "C" int dspmap_get_cost_weights(dspmap_t* m, unsigned char* out) {
    if (!m) return DSPMAP_E_ARG;
    if (!out) return dspmap_fail(m, DSPMAP_E_ARG, "cost weights: NULL output array");
    const int rc = cost_ready(m, "dspmap_get_cost_weights");
    if (rc != DSPMAP_OK) return rc;
    return read_back(m, out, m->ly.cf_weight, (size_t)m->d.v_glob);
}
// (dspmap_cost_paths*: with the reach paths, paths_host / paths_device above)
// test hook: all L layers of the VALID distance field are replaced by the caller's floats
extern "C" int dspmap_debug_set_distance_field(dspmap_t* m, const float* layers) {
    if (!m) return DSPMAP_E_ARG;
    if (!layers) return dspmap_fail(m, DSPMAP_E_ARG, "set distance field: NULL layer array");
    const size_t total = (size_t)(m->d.T + 1) * (size_t)m->d.v_glob;
    for (size_t i = 0; i < total; ++i)
        if (!(layers[i] >= 0.f && layers[i] < INFINITY))
            return dspmap_fail(m, DSPMAP_E_ARG, "set distance field: value %zu = %g is NaN, negative or infinite", i, (double)layers[i]);
    int rc = whole_map_check(m, "set distance field", "");
    if (rc != DSPMAP_OK) return rc;
    if ((rc = dist_field_ready(m, "dspmap_debug_set_distance_field")) != DSPMAP_OK) return rc;
    dspmap_layers_stale(m->ly, LAYERS_DISTANCE_CHANGED);
    HIPCHK(m, hipMemcpyAsync(m->ly.df_field, layers, sizeof(float) * total, hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));   // (the caller's array is free again)
    return DSPMAP_OK;
}

// --------------------------------------------------- the end of the handle
void dspmap_layers_free(dspmap* m, const std::function<void(hipError_t, const char*)>& chk) {
    const LayerState& l = m->ly;
    for (void* q : {(void*)l.q_buf, (void*)l.df_field, (void*)l.df_g8, (void*)l.df_h16, (void*)l.nr_near, (void*)l.nr_dist, (void*)l.nr_x8, (void*)l.nr_key32, (void*)l.cg_bits, (void*)l.cg_tmp, (void*)l.rf_field,
                    (void*)l.rf_sets, (void*)l.tl_hist, (void*)l.tl_last, (void*)l.cf_field, (void*)l.cf_sets, (void*)l.cf_weight, (void*)l.cf_wk, (void*)l.cf_occ, (void*)l.fc_field, (void*)l.fc_acc, (void*)l.kn_stamp, (void*)l.vw_dirs0, (void*)l.vs_masks, (void*)l.vs_aux,
                    (void*)l.fr_grid, (void*)l.fr_cells, (void*)l.fr_counts, (void*)l.fr_item_free, (void*)l.fr_dense, (void*)l.fr_blocks,
                    (void*)l.fr_tiles, (void*)l.ob_parent, (void*)l.ob_root, (void*)l.ob_labels, (void*)l.ob_tiles, (void*)l.ob_counts,
                    (void*)l.ob_objects, (void*)l.tk_labels, (void*)l.tk_objects, (void*)l.tk_tracks[0], (void*)l.tk_tracks[1], (void*)l.tk_shift,
                    (void*)l.tk_tiles, (void*)l.tk_zero, (void*)l.tk_counts})
        if (q) chk(hipFree(q), "hipFree");
}
