// dspmap_depth.hip -- depth images straight to the map: back-projection + voxel-grid centroid filter + axis swap + crop + cap on the device
// (dspmap_preprocess_depth, dspmap_update_depth_device, dspmap_update_depth; semantics next to them in include/dspmap.h).
//
// What dspmap_preprocess.hip does for a cloud that already lies in memory (12 B per point, one thread per point, four float atomics each)
// is done here from the sensor's own data: k_dp_accumulate reads the image (2 B or 4 B per pixel), back-projects in registers and
// reduces BEFORE memory:
//   * a workgroup owns a tile of DP_TW x DP_TH (64 x 16) used pixels; a wave takes one row of 64 consecutive pixels at a time (one coalesced
//     128-B / 256-B segment), four rows in all;
//   * neighbouring pixels of a row fall into the same leaf (a 0.1 m leaf at 1 m covers ~32 x 32 pixels, at 3 m ~10 x 10): the wave sums
//     every run of equal leaf among adjacent lanes with a segmented scan over the lanes (six shuffle steps), the run's last lane owns the sum;
//   * the run sums of the tile's 16 rows meet in an LDS table keyed by leaf (DP_TAB entries, open addressing, a few probes);
//   * the table is flushed with ONE 64-bit integer atomic per (tile, leaf) and coordinate, and one for the count.  A run that finds no
//     place in the table (a tile that touches more leaves than it holds: tiny leaves, far noisy surfaces) adds its sums to memory itself.
// The sums are integers (llrint(p * 2^20) per coordinate, 64 bit): every path adds the same integers, so the leaf sums -- and with them
// the filtered cloud -- do not depend on the tile shape, the order of the waves or which path a run took.  |S| < 2^63 holds for any
// image of up to 2^24 x 2^24 pixels of coordinates below 2^15 m; the map box keeps them far below that.
// k_dp_count / k_pp_scan / k_dp_emit mirror the cloud path on the new accumulator layout {count[cell]}, {Sx, Sy, Sz}[cell]: the two
// sweeps over the lattice read 4 B per leaf (the sums only of occupied leaves), and the emit sweep zeroes what it has read, so that the
// next frame starts from a clean grid without a 20-MB memset.
#include "dspmap_device.h"
#include "dspmap_internal.h"

#include <cmath>
#include <cstring>

#define DP_TPB 256
#define DP_TW 64                      // used pixels per tile row = lanes of a wave
#define DP_TH 16                      // tile rows
#define DP_ROWS (DP_TH / (DP_TPB / 64))   // rows per wave
#define DP_TAB 512                    // LDS table entries (power of two)
#define DP_PROBES 8
#define DP_MAX_CELLS (1ll << 27)      // as PP_MAX_CELLS: finer lattices over the map box are refused
#define DP_SCALE 1048576.0            // 2^20 fixed-point units per metre
#define DP_MAX_SIDE (1 << 24)         // (float)u is exact below

struct DPGrid {
    int div[3];
    float min_bf[3];                  // (float)min_b
    float inv_leaf;
    long long cells;
};
struct DPArgs {
    int ws, hs, step;                 // used columns / rows, stride between them in pixels
    int stride_bytes, format;
    int tiles_x;
    float fx, fy, cx, cy, scale, min_d, max_d;
};

__device__ __forceinline__ u64 lanemask_le() { return lanemask_lt() | (1ull << lane_id()); }

__global__ void __launch_bounds__(DP_TPB) k_dp_accumulate(const unsigned char* __restrict__ img, DPArgs a, DPGrid g,
                                                          long long* __restrict__ sum, int* __restrict__ cnt, int* __restrict__ n_valid) {
    __shared__ int s_key[DP_TAB];
    __shared__ u64 s_sum[3][DP_TAB];
    __shared__ int s_cnt[DP_TAB];
    __shared__ int s_valid;
    for (int e = threadIdx.x; e < DP_TAB; e += DP_TPB) { s_key[e] = -1; s_sum[0][e] = 0; s_sum[1][e] = 0; s_sum[2][e] = 0; s_cnt[e] = 0; }
    if (threadIdx.x == 0) s_valid = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int su = tx * DP_TW + lane;             // used column
    const int u = su * a.step;                    // pixel column
    const float xu = __fsub_rn((float)u, a.cx);
    int valid = 0;
#pragma unroll
    for (int r = 0; r < DP_ROWS; ++r) {
        const int sv = ty * DP_TH + wave * DP_ROWS + r;   // used row (wave-uniform)
        if (sv >= a.hs) break;                    // (wave-uniform: the shuffles below stay converged)
        const int v = sv * a.step;
        float rawf = 0.f;
        bool ok = false;
        if (su < a.ws) {
            const unsigned char* row = img + (size_t)v * (size_t)a.stride_bytes;
            if (a.format == DSPMAP_DEPTH_U16) {
                const unsigned short w = reinterpret_cast<const unsigned short*>(row)[u];
                rawf = (float)w;
                ok = w != 0;
            } else {
                rawf = reinterpret_cast<const float*>(row)[u];
                ok = isfinite(rawf) && rawf > 0.f;
            }
        }
        const float d = __fmul_rn(rawf, a.scale);
        ok = ok && d >= a.min_d && d <= a.max_d;
        valid += (int)__popcll(__ballot(ok));
        int cell = -1;
        long long qx = 0, qy = 0, qz = 0;
        if (ok) {
            const float X = __fdiv_rn(__fmul_rn(xu, d), a.fx);
            const float Y = __fdiv_rn(__fmul_rn(__fsub_rn((float)v, a.cy), d), a.fy);
            const float Z = d;
            if (isfinite(X) && isfinite(Y) && isfinite(Z)) {
                // voxel_grid.hpp: ijk = static_cast<int>(std::floor(p * inverse_leaf_size) - static_cast<float>(min_b)); the range test is
                // made on the float (an integer value, or too large to matter) so that no out-of-range conversion happens
                const float f0 = __fsub_rn(floorf(__fmul_rn(X, g.inv_leaf)), g.min_bf[0]);
                const float f1 = __fsub_rn(floorf(__fmul_rn(Y, g.inv_leaf)), g.min_bf[1]);
                const float f2 = __fsub_rn(floorf(__fmul_rn(Z, g.inv_leaf)), g.min_bf[2]);
                if (f0 >= 0.f && f0 < (float)g.div[0] && f1 >= 0.f && f1 < (float)g.div[1] && f2 >= 0.f && f2 < (float)g.div[2]) {
                    cell = (int)f0 + ((int)f1 + (int)f2 * g.div[1]) * g.div[0];   // (cells <= 2^27)
                    qx = __double2ll_rn((double)X * DP_SCALE);
                    qy = __double2ll_rn((double)Y * DP_SCALE);
                    qz = __double2ll_rn((double)Z * DP_SCALE);
                }
            }
        }
        // runs of equal leaf among adjacent lanes: segmented inclusive scan, the run's last lane ends up with the run's sums
        const int left = __shfl_up(cell, 1);
        const bool head = lane == 0 || left != cell;
        const u64 heads = __ballot(head);
        const int h = 63 - (int)__clzll(heads & lanemask_le());   // first lane of this lane's run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long tx_ = __shfl_up(qx, off), ty_ = __shfl_up(qy, off), tz_ = __shfl_up(qz, off);
            if (lane - off >= h) { qx += tx_; qy += ty_; qz += tz_; }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && cell >= 0) {
            const int n = lane - h + 1;
            const unsigned hs = ((unsigned)cell * 2654435761u) >> 23;   // 9 bits
            bool done = false;
            for (int p = 0; p < DP_PROBES && !done; ++p) {
                const int e = (int)((hs + (unsigned)p) & (DP_TAB - 1));
                const int prev = atomicCAS(&s_key[e], -1, cell);
                if (prev == -1 || prev == cell) {
                    atomicAdd(&s_sum[0][e], (u64)qx); atomicAdd(&s_sum[1][e], (u64)qy); atomicAdd(&s_sum[2][e], (u64)qz);
                    atomicAdd(&s_cnt[e], n);
                    done = true;
                }
            }
            if (!done) {
                u64* s = reinterpret_cast<u64*>(sum + 3 * (size_t)cell);
                atomicAdd(s, (u64)qx); atomicAdd(s + 1, (u64)qy); atomicAdd(s + 2, (u64)qz);
                atomicAdd(cnt + cell, n);
            }
        }
    }
    if (lane == 0 && valid) atomicAdd(&s_valid, valid);
    __syncthreads();
    for (int e = threadIdx.x; e < DP_TAB; e += DP_TPB) {
        const int cell = s_key[e];
        if (cell < 0) continue;
        u64* s = reinterpret_cast<u64*>(sum + 3 * (size_t)cell);
        atomicAdd(s, s_sum[0][e]); atomicAdd(s + 1, s_sum[1][e]); atomicAdd(s + 2, s_sum[2][e]);
        atomicAdd(cnt + cell, s_cnt[e]);
    }
    if (threadIdx.x == 0 && s_valid) atomicAdd(n_valid, s_valid);
}

// centroid of a leaf from its integer sums, axis swap (:321-323), open-box crop (:190-197,325)
__device__ __forceinline__ bool dp_point(int n, const long long* __restrict__ s, float hx, float hy, float hz, float& x, float& y, float& z) {
    const double dn = (double)n;
    const float cx = (float)(__ddiv_rn((double)s[0], dn) * (1.0 / DP_SCALE));
    const float cy = (float)(__ddiv_rn((double)s[1], dn) * (1.0 / DP_SCALE));
    const float cz = (float)(__ddiv_rn((double)s[2], dn) * (1.0 / DP_SCALE));
    x = cz; y = -cx; z = -cy;
    return x > -hx && x < hx && y > -hy && y < hy && z > -hz && z < hz;
}
__global__ void __launch_bounds__(DP_TPB) k_dp_count(const int* __restrict__ cnt, const long long* __restrict__ sum, long long cells, float hx,
                                                     float hy, float hz, int* __restrict__ blk_cnt, int* __restrict__ n_leaves) {
    __shared__ int s_c[DP_TPB / 64], s_l[DP_TPB / 64];
    const long long c = (long long)blockIdx.x * DP_TPB + threadIdx.x;
    float x, y, z;
    bool leaf = false, keep = false;
    if (c < cells) {
        const int n = cnt[c];
        leaf = n > 0;
        if (leaf) keep = dp_point(n, sum + 3 * c, hx, hy, hz, x, y, z);
    }
    const u64 bk = __ballot(keep), bl = __ballot(leaf);
    if (lane_id() == 0) { s_c[threadIdx.x >> 6] = (int)__popcll(bk); s_l[threadIdx.x >> 6] = (int)__popcll(bl); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0, tl = 0;
        for (int k = 0; k < DP_TPB / 64; ++k) { t += s_c[k]; tl += s_l[k]; }
        blk_cnt[blockIdx.x] = t;
        if (tl) atomicAdd(n_leaves, tl);
    }
}
// exclusive scan of the per-block counts (the same scan as k_pp_scan of the cloud path, which dspmap_preprocess.hip keeps to itself)
__global__ void __launch_bounds__(1024) k_dp_scan(int* __restrict__ blk_cnt, int nblk, int* __restrict__ total) {
    __shared__ int s_w[16];
    __shared__ int s_run;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + tid;
        const int v = i < nblk ? blk_cnt[i] : 0;
        const int inc = wave_incl_scan_i(v);
        if (l == 63) s_w[w] = inc;
        __syncthreads();
        int off = s_run;
        for (int k = 0; k < w; ++k) off += s_w[k];
        if (i < nblk) blk_cnt[i] = off + inc - v;
        __syncthreads();
        if (tid == 1023) s_run = off + inc;
        __syncthreads();
    }
    if (tid == 0) *total = s_run;
}
// writes the kept centroids in lattice order and leaves the grid zeroed behind it
__global__ void __launch_bounds__(DP_TPB) k_dp_emit(int* __restrict__ cnt, long long* __restrict__ sum, long long cells, float hx, float hy,
                                                    float hz, const int* __restrict__ blk_off, int max_points, float* __restrict__ out) {
    __shared__ int s_c[DP_TPB / 64];
    const long long c = (long long)blockIdx.x * DP_TPB + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    bool keep = false;
    if (c < cells) {
        const int n = cnt[c];
        if (n > 0) {
            keep = dp_point(n, sum + 3 * c, hx, hy, hz, x, y, z);
            cnt[c] = 0;
            sum[3 * c] = 0; sum[3 * c + 1] = 0; sum[3 * c + 2] = 0;
        }
    }
    const u64 b = __ballot(keep);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) s_c[w] = (int)__popcll(b);
    __syncthreads();
    int off = blk_off[blockIdx.x];
    for (int k = 0; k < w; ++k) off += s_c[k];
    if (keep) {
        const int pos = off + (int)__popcll(b & lanemask_lt());
        if (pos < max_points) {   // :332: the loop stops once the buffer is full
            out[3 * (size_t)pos] = x; out[3 * (size_t)pos + 1] = y; out[3 * (size_t)pos + 2] = z;
        }
    }
}

// ---- host side
static int dp_elem_bytes(int format) { return format == DSPMAP_DEPTH_U16 ? 2 : 4; }
static long long dp_row_bytes(const dspmap_camera* cam) {
    return cam->row_stride_bytes ? (long long)cam->row_stride_bytes : (long long)cam->width * dp_elem_bytes(cam->format);
}
// argument checks of the three entry points: before READY, so that they hold without a device
static int dp_check(dspmap* m, const dspmap_camera* cam, const void* image, float leaf, int max_points) {
    if (!m) return DSPMAP_E_ARG;
    if (!cam) return dspmap_fail(m, DSPMAP_E_ARG, "depth: NULL camera");
    if (!image) return dspmap_fail(m, DSPMAP_E_ARG, "depth: NULL image");
    if (cam->width < 1 || cam->height < 1 || cam->width > DP_MAX_SIDE || cam->height > DP_MAX_SIDE)
        return dspmap_fail(m, DSPMAP_E_ARG, "depth: image of %d x %d pixels", cam->width, cam->height);
    // (the upper bound keeps width + step - 1 on the host and su * step in k_dp_accumulate, lanes beyond ws included, inside an int:
    //  su <= ws + 62 and ws * step < width + step, so su * step < 2^25 + 62 * 2^24 < 2^31)
    if (cam->pixel_step < 1 || cam->pixel_step > DP_MAX_SIDE)
        return dspmap_fail(m, DSPMAP_E_ARG, "depth: pixel_step %d outside 1 .. %d", cam->pixel_step, DP_MAX_SIDE);
    if (cam->format != DSPMAP_DEPTH_U16 && cam->format != DSPMAP_DEPTH_F32) return dspmap_fail(m, DSPMAP_E_ARG, "depth: unknown format %d", cam->format);
    const int eb = dp_elem_bytes(cam->format);
    if (cam->row_stride_bytes != 0 && ((long long)cam->row_stride_bytes < (long long)cam->width * eb || cam->row_stride_bytes % eb != 0))
        return dspmap_fail(m, DSPMAP_E_ARG, "depth: row stride of %d bytes for rows of %d x %d bytes", cam->row_stride_bytes, cam->width, eb);
    if (!(std::isfinite(cam->fx) && cam->fx > 0.f && std::isfinite(cam->fy) && cam->fy > 0.f))
        return dspmap_fail(m, DSPMAP_E_ARG, "depth: focal lengths %g, %g", (double)cam->fx, (double)cam->fy);
    if (!(std::isfinite(cam->cx) && std::isfinite(cam->cy))) return dspmap_fail(m, DSPMAP_E_ARG, "depth: principal point %g, %g", (double)cam->cx, (double)cam->cy);
    if (!(std::isfinite(cam->depth_scale) && cam->depth_scale > 0.f)) return dspmap_fail(m, DSPMAP_E_ARG, "depth: depth_scale %g", (double)cam->depth_scale);
    if (!(cam->min_depth <= cam->max_depth)) return dspmap_fail(m, DSPMAP_E_ARG, "depth: range [%g, %g]", (double)cam->min_depth, (double)cam->max_depth);
    if (!(leaf > 0.f)) return dspmap_fail(m, DSPMAP_E_ARG, "depth: leaf size %g", (double)leaf);
    if (max_points < 0) return dspmap_fail(m, DSPMAP_E_ARG, "depth: max_points %d", max_points);
    return DSPMAP_OK;
}

// image (device memory) -> at most max_points filtered points in out_dev; synchronous.  tot = {kept by the crop, leaves, valid pixels}
static int dp_ingest(dspmap* m, const dspmap_camera* cam, const void* depth_dev, float leaf, int max_points, float* out_dev, int tot[3]) {
    const float hx = m->d.half_x, hy = m->d.half_y, hz = m->d.half_z;
    const float hin[3] = {hy, hz, hx};   // the map box in the camera frame: x_map = z_cam, y_map = -x_cam, z_map = -y_cam (:321-323)
    DPGrid g;
    g.inv_leaf = 1.0f / leaf;            // inverse_leaf_size_ = Array4f::Ones() / leaf_size_
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        const float flo = floorf(-hin[a] * g.inv_leaf), fhi = floorf(hin[a] * g.inv_leaf);
        if (!(fhi - flo + 1.f <= (float)DP_MAX_CELLS))
            return dspmap_fail(m, DSPMAP_E_ARG, "leaf size %.4g too small for the map box (more than %lld leaves)", (double)leaf, (long long)DP_MAX_CELLS);
        const int lo = (int)flo, hi = (int)fhi;
        g.min_bf[a] = (float)lo;
        g.div[a] = hi - lo + 1;
        cells *= (long long)g.div[a];
        if (cells > DP_MAX_CELLS)
            return dspmap_fail(m, DSPMAP_E_ARG, "leaf size %.4g too small for the map box (more than %lld leaves)", (double)leaf, (long long)DP_MAX_CELLS);
    }
    g.cells = cells;
    DPArgs a;
    a.step = cam->pixel_step;
    a.ws = (cam->width + a.step - 1) / a.step;
    a.hs = (cam->height + a.step - 1) / a.step;
    a.stride_bytes = (int)dp_row_bytes(cam);
    a.format = cam->format;
    a.tiles_x = (a.ws + DP_TW - 1) / DP_TW;
    const long long tiles = (long long)a.tiles_x * ((a.hs + DP_TH - 1) / DP_TH);
    if (tiles > 0x7fffffffll) return dspmap_fail(m, DSPMAP_E_ARG, "depth: %lld tiles of %d x %d pixels exceed INT_MAX", tiles, DP_TW, DP_TH);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.scale = cam->depth_scale; a.min_d = cam->min_depth; a.max_d = cam->max_depth;
    if (!m->dp_tot) HIPCHK(m, hipMalloc((void**)&m->dp_tot, 3 * sizeof(int)));
    if ((size_t)cells > m->dp_cells_cap) {
        if (m->dp_sum) (void)hipFree(m->dp_sum);
        if (m->dp_cnt) (void)hipFree(m->dp_cnt);
        if (m->dp_blk) (void)hipFree(m->dp_blk);
        m->dp_sum = nullptr; m->dp_cnt = nullptr; m->dp_blk = nullptr; m->dp_cells_cap = 0;
        HIPCHK(m, hipMalloc((void**)&m->dp_sum, sizeof(long long) * 3 * (size_t)cells));
        HIPCHK(m, hipMalloc((void**)&m->dp_cnt, sizeof(int) * (size_t)cells));
        HIPCHK(m, hipMalloc((void**)&m->dp_blk, sizeof(int) * ((size_t)(cells + DP_TPB - 1) / DP_TPB + 1)));
        m->dp_cells_cap = (size_t)cells;
        m->dp_dirty = true;
    }
    if (m->dp_dirty) {   // a new grid, or a call that did not reach its end: every later frame finds the grid zeroed by k_dp_emit
        HIPCHK(m, hipMemsetAsync(m->dp_sum, 0, sizeof(long long) * 3 * m->dp_cells_cap, m->stream));
        HIPCHK(m, hipMemsetAsync(m->dp_cnt, 0, sizeof(int) * m->dp_cells_cap, m->stream));
    }
    m->dp_dirty = true;
    HIPCHK(m, hipMemsetAsync(m->dp_tot, 0, 3 * sizeof(int), m->stream));
    hipLaunchKernelGGL(k_dp_accumulate, dim3((unsigned)tiles), dim3(DP_TPB), 0, m->stream, (const unsigned char*)depth_dev, a, g, m->dp_sum, m->dp_cnt,
                       m->dp_tot + 2);
    const int nblk = (int)((cells + DP_TPB - 1) / DP_TPB);
    hipLaunchKernelGGL(k_dp_count, dim3(nblk), dim3(DP_TPB), 0, m->stream, m->dp_cnt, m->dp_sum, cells, hx, hy, hz, m->dp_blk, m->dp_tot + 1);
    hipLaunchKernelGGL(k_dp_scan, dim3(1), dim3(1024), 0, m->stream, m->dp_blk, nblk, m->dp_tot);
    hipLaunchKernelGGL(k_dp_emit, dim3(nblk), dim3(DP_TPB), 0, m->stream, m->dp_cnt, m->dp_sum, cells, hx, hy, hz, m->dp_blk, max_points, out_dev);
    HIPCHK(m, hipMemcpyAsync(tot, m->dp_tot, 3 * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipGetLastError());
    m->dp_dirty = false;
    if (tot[0] > max_points) tot[0] = max_points;
    return DSPMAP_OK;
}

extern "C" int dspmap_preprocess_depth(dspmap_t* m, const dspmap_camera* cam, const void* depth_dev, float leaf, int max_points,
                                       float* out_dev, int* n_out, int* n_leaves_out, int* n_valid_out) {
    int rc = dp_check(m, cam, depth_dev, leaf, max_points);
    if (rc != DSPMAP_OK) return rc;
    if ((max_points > 0 && !out_dev) || !n_out) return dspmap_fail(m, DSPMAP_E_ARG, "depth: NULL output");
    READY(m);
    int tot[3] = {0, 0, 0};
    rc = dp_ingest(m, cam, depth_dev, leaf, max_points, out_dev, tot);
    if (rc != DSPMAP_OK) return rc;
    *n_out = tot[0];
    if (n_leaves_out) *n_leaves_out = tot[1];
    if (n_valid_out) *n_valid_out = tot[2];
    return DSPMAP_OK;
}

// gate -> ingest into the handle's cloud buffer -> the frame of dspmap_update_device on that buffer
static int dp_frame(dspmap* m, const dspmap_camera* cam, const void* depth, bool host_image, float leaf, int max_points, const float pos[3],
                    double stamp, const float q[4]) {
    { const int rq = dspmap_check_estimator_queue(m); if (rq != DSPMAP_OK) return rq; }
    float dp[3], dt;
    if (!dspmap_gate_and_delta(m, pos, stamp, q, dp, &dt)) return DSPMAP_REJECTED;   // before anything is queued
    const void* depth_dev = depth;
    if (host_image) {
        const size_t bytes = (size_t)dp_row_bytes(cam) * (size_t)(cam->height - 1) + (size_t)cam->width * (size_t)dp_elem_bytes(cam->format);
        if (bytes > m->dp_img_bytes) {   // (every earlier use of the buffers has ended: the ingest is synchronous)
            if (m->dp_img) (void)hipFree(m->dp_img);
            if (m->dp_img_pin) (void)hipHostFree(m->dp_img_pin);
            m->dp_img = nullptr; m->dp_img_pin = nullptr; m->dp_img_bytes = 0; m->dp_img_pin_bytes = 0;
            HIPCHK(m, hipMalloc(&m->dp_img, bytes));
            HIPCHK(m, hipHostMalloc(&m->dp_img_pin, bytes));
            m->dp_img_bytes = bytes; m->dp_img_pin_bytes = bytes;
        }
        memcpy(m->dp_img_pin, depth, bytes);
        HIPCHK(m, hipMemcpyAsync(m->dp_img, m->dp_img_pin, bytes, hipMemcpyHostToDevice, m->stream));
        depth_dev = m->dp_img;
    }
    if (max_points > m->dp_out_cap || !m->dp_out) {
        HIPCHK(m, hipStreamSynchronize(m->stream));   // an earlier frame may still read the buffer
        if (m->dp_out) (void)hipFree(m->dp_out);
        m->dp_out = nullptr; m->dp_out_cap = 0;
        const int cap = max_points > 0 ? max_points : 1;
        HIPCHK(m, hipMalloc((void**)&m->dp_out, sizeof(float) * 3 * (size_t)cap));
        m->dp_out_cap = cap;
    }
    int tot[3] = {0, 0, 0};
    const int rc = dp_ingest(m, cam, depth_dev, leaf, max_points, m->dp_out, tot);   // (queued behind the last frame, which read dp_out)
    if (rc != DSPMAP_OK) return rc;
    return dspmap_device_frame(m, tot[0], m->dp_out, 0, nullptr, dp, dt, q);
}

extern "C" int dspmap_update_depth_device(dspmap_t* m, const dspmap_camera* cam, const void* depth_dev, float leaf, int max_points,
                                          const float pos[3], double stamp, const float q[4]) {
    const int rc = dp_check(m, cam, depth_dev, leaf, max_points);
    if (rc != DSPMAP_OK) return rc;
    if (!pos || !q) return dspmap_fail(m, DSPMAP_E_ARG, "depth: NULL pose");
    READY(m);
    return dp_frame(m, cam, depth_dev, false, leaf, max_points, pos, stamp, q);
}

extern "C" int dspmap_update_depth(dspmap_t* m, const dspmap_camera* cam, const void* depth_host, float leaf, int max_points,
                                   const float pos[3], double stamp, const float q[4]) {
    const int rc = dp_check(m, cam, depth_host, leaf, max_points);
    if (rc != DSPMAP_OK) return rc;
    if (!pos || !q) return dspmap_fail(m, DSPMAP_E_ARG, "depth: NULL pose");
    READY(m);
    return dp_frame(m, cam, depth_host, true, leaf, max_points, pos, stamp, q);
}
