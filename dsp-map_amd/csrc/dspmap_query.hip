// dspmap_query.hip -- read-only queries of the map's occupancy and future status at arbitrary points (dspmap_query_occupancy*,
// dspmap_trajectory_risk*; semantics next to them in include/dspmap.h).  The reference has no counterpart: its only readouts are
// whole-grid copies (getOccupancyMapWithFutureStatus :405-426), which a planner sampling motion primitives would have to index itself.
//
// What a sample reads, in place and in storage order (no [V][T] combine, no host copy):
//   t < 0 (or T == 0)  res4[lv].x                         = voxels_objects_number[v][0]  (dspmap_get_results)
//   t >= 0             fut_status_at(lv, k(t))            = the grid dspmap_get_future returns, bit for bit (the helper is the one
//                                                           k_future_combine uses), or 0 while a clear is pending (:397-400, :420-424)
// Nothing is written but the caller's output: the accumulators are not cleared and the handle's clear flag is left as it is.
//
// Lane mapping: ONE THREAD PER SAMPLE at every radius.  Every lane's candidate box has the same (2K + 1)^3 lattice points (only the
// clamping at the map's faces differs), so the three loops run the same trip counts across the wave and the lanes stay converged.
// A candidate costs ~10 VALU operations and at most two gathers (one for t < 0); a whole plane or row of the box is skipped with one
// compare once its partial distance exceeds r^2 (exact: fp32 rounding is monotone).  131 072 samples are 2 048 waves, two per SIMD of
// the 256 CUs, with 12 - 31 VGPRs (8 waves / SIMD possible).  A wave per sample with a DPP max reduction over the box would leave most
// of its 64 lanes idle at the radii a planner uses (r = 0: one voxel; 0.3 m at 0.15 m: ~33 of 343 candidates pass) and multiply the
// waves by 64; it could only pay at the widest admitted radius (8 voxels, 6 859 candidates).  Samples of one trajectory sit in
// neighbouring lanes, so their gathers share cache lines.
// The r = 0 path is its own instantiation: one 16-B sample load, voxel_of, and the gathers of the own voxel.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"

#define Q_TPB 256

// (q_horizon, the horizon k(t) a sample reads, lives in dspmap_device.h: dspmap_distance.hip picks its layer with it too)
__device__ __forceinline__ float q_mass(const MapDims& d, const DevState& s, int lv, int k, int fut_zero) {
    if (k < 0) return s.res4[lv].x;
    return fut_zero ? 0.f : fut_status_at(d, s, lv, k);
}
// voxel centre along one axis, dspmap_voxel_center's arithmetic (getVoxelPositionFromIndexPublic :1556-1572), any integer index
__device__ __forceinline__ float q_centre(int i, float res, float corr) { return __fadd_rn(__fmul_rn((float)i, res), corr); }
// candidate lattice indices of one axis: [lo, hi] around p, K steps either side, clamped to [-1, n] (a lattice point beyond -1 / n is
// never closer to a point inside the map than the one at -1 / n -- and a point outside the map already reads `outside`)
__device__ __forceinline__ void q_span(float p, float corr, float res, int n, int K, int& lo, int& hi) {
    float f = floorf(__fdiv_rn(__fsub_rn(p, corr), res));
    f = fminf(fmaxf(f, (float)(-K - 2)), (float)(n + K + 1));   // (infinite p: the box ends up empty)
    const int ic = (int)f;
    lo = max(ic - K, -1);
    hi = min(ic + K, n);
}

// one sample's value; *outside = the point is outside the map or a coordinate / t is NaN (dspmap_risk::n_outside)
template <bool LATTICE>
__device__ __forceinline__ float q_value(const MapDims& d, const DevState& s, const QueryArgs& a, float4 q, bool& outside) {
    if (q.x != q.x || q.y != q.y || q.z != q.z || q.w != q.w) { outside = true; return a.outside; }   // (voxel_of lets NaN through)
    float px = q.x, py = q.y, pz = q.z;
    origin_apply(a.org, px, py, pz);
    const int k = q_horizon(d, q.w);
    const int nzl = d.z_hi - d.z_lo;
    float best = -INFINITY;
    int g;
    if (voxel_of(d, px, py, pz, g)) {   // getPointVoxelsIndexPublic's voxel
        outside = false;
        const int lv = lv_of_g(d, g);
        if (lv >= 0) best = q_mass(d, s, lv, k, a.fut_zero);
    } else {
        outside = true;
        best = a.outside;
    }
    if (!LATTICE) return best;
    int x0, x1, y0, y1, z0, z1;
    q_span(px, a.cx, d.res, d.nx, a.K, x0, x1);
    q_span(py, a.cy, d.res, d.ny, a.K, y0, y1);
    q_span(pz, a.cz, d.res, d.nz, a.K, z0, z1);
    for (int iz = z0; iz <= z1; ++iz) {
        const float dz = __fsub_rn(q_centre(iz, d.res, a.cz), pz);
        const float dz2 = __fmul_rn(dz, dz);
        if (dz2 > a.r2) continue;   // d2 = fl(fl(dx2 + dy2) + dz2) >= dz2
        const bool z_in = (unsigned)iz < (unsigned)d.nz;
        const int zl = iz - d.z_lo;
        const bool z_mine = (unsigned)zl < (unsigned)nzl;
        for (int iy = y0; iy <= y1; ++iy) {
            const float dy = __fsub_rn(q_centre(iy, d.res, a.cy), py);
            const float dy2 = __fmul_rn(dy, dy);
            if (__fadd_rn(dy2, dz2) > a.r2) continue;   // d2 >= fl(dy2 + dz2)
            const bool yz_in = z_in && (unsigned)iy < (unsigned)d.ny;
            for (int ix = x0; ix <= x1; ++ix) {
                const float dx = __fsub_rn(q_centre(ix, d.res, a.cx), px);
                const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), dy2), dz2);
                if (!(d2 <= a.r2)) continue;
                if (!(yz_in && (unsigned)ix < (unsigned)d.nx)) best = fmaxf(best, a.outside);
                else if (z_mine) best = fmaxf(best, q_mass(d, s, lv_of_xyz(d, ix, iy, zl), k, a.fut_zero));
            }
        }
    }
    return best;
}

template <bool LATTICE, bool FLAGS>
__global__ void __launch_bounds__(Q_TPB) k_query(MapDims d, DevState s, QueryArgs a, int n, const float4* __restrict__ q,
                                                  float* __restrict__ out, unsigned char* __restrict__ out_flag) {
    const unsigned i = blockIdx.x * Q_TPB + threadIdx.x;   // (unsigned: n may come within a block of INT_MAX)
    if (i >= (unsigned)n) return;
    bool outside;
    const float v = q_value<LATTICE>(d, s, a, q[i], outside);
    out[i] = v;
    if (FLAGS) out_flag[i] = outside ? 1 : 0;
}

// One lane per trajectory: the sum is taken sequentially in sample order (the fp32 sum a numpy float32 loop computes).  The
// block's Q_TPB trajectories are staged in LDS RISK_CHUNK samples at a time: consecutive lanes load consecutive samples of a
// trajectory (RISK_CHUNK * 4 = 128-byte segments), instead of every lane reading its own row n_samples * 4 bytes from its
// neighbour's; each lane then walks its own LDS row (33 floats apart: no bank conflicts).
#define RISK_CHUNK 32
__global__ void __launch_bounds__(Q_TPB) k_risk_reduce(int n_traj, int n_samples, const float* __restrict__ v,
                                                        const unsigned char* __restrict__ flag, float threshold, dspmap_risk* __restrict__ out) {
    __shared__ float sv[Q_TPB][RISK_CHUNK + 1];
    __shared__ unsigned char sf[Q_TPB][RISK_CHUNK + 4];
    const unsigned t0 = blockIdx.x * Q_TPB;
    const int nt = (int)min((unsigned)Q_TPB, (unsigned)n_traj - t0);   // trajectories of this block
    const int l = threadIdx.x;
    float sum = 0.f, mx = -INFINITY;
    int first = -1, n_out = 0;
    for (int j0 = 0; j0 < n_samples; j0 += RISK_CHUNK) {
        const int cn = min(RISK_CHUNK, n_samples - j0);
        __syncthreads();   // the previous chunk is consumed
        for (int e = l; e < nt * cn; e += Q_TPB) {
            const int row = e / cn, col = e - row * cn;
            const size_t g = (size_t)(t0 + row) * n_samples + j0 + col;
            sv[row][col] = v[g];
            sf[row][col] = flag[g];
        }
        __syncthreads();
        if (l < nt) {
            for (int j = 0; j < cn; ++j) {
                const float x = sv[l][j];
                sum = __fadd_rn(sum, x);
                mx = fmaxf(mx, x);
                if (first < 0 && x > threshold) first = j0 + j;
                n_out += sf[l][j];
            }
        }
    }
    if (l < nt) {
        dspmap_risk r;
        r.sum = sum; r.max = mx; r.first_over = first; r.n_outside = n_out;
        out[t0 + l] = r;
    }
}

static dim3 q_grid(long long n) { return dim3((unsigned)((n + Q_TPB - 1) / Q_TPB)); }   // (64-bit: n up to INT_MAX)

void launch_query(const LaunchCtx& c, const QueryArgs& a, int n, const float4* q, float* out, unsigned char* out_flag) {
    if (n <= 0) return;
    const dim3 g = q_grid(n);
    if (a.K > 0) {
        if (out_flag) hipLaunchKernelGGL((k_query<true, true>), g, dim3(Q_TPB), 0, c.stream, c.d, c.s, a, n, q, out, out_flag);
        else hipLaunchKernelGGL((k_query<true, false>), g, dim3(Q_TPB), 0, c.stream, c.d, c.s, a, n, q, out, out_flag);
    } else {
        if (out_flag) hipLaunchKernelGGL((k_query<false, true>), g, dim3(Q_TPB), 0, c.stream, c.d, c.s, a, n, q, out, out_flag);
        else hipLaunchKernelGGL((k_query<false, false>), g, dim3(Q_TPB), 0, c.stream, c.d, c.s, a, n, q, out, out_flag);
    }
}
void launch_risk_reduce(const LaunchCtx& c, int n_traj, int n_samples, const float* v, const unsigned char* flag, float threshold,
                        dspmap_risk* out) {
    if (n_traj <= 0) return;
    hipLaunchKernelGGL(k_risk_reduce, q_grid(n_traj), dim3(Q_TPB), 0, c.stream, n_traj, n_samples, v, flag,
                       threshold, out);
}
