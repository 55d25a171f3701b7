// dspmap_known.hip -- the known-space layer (dspmap_known_integrate, dspmap_get_known, dspmap_query_known*, dspmap_mask_cast_grid,
// dspmap_known_stats; semantics next to them in include/dspmap.h).  The map reports a mass of 0 both for a voxel the filter has looked
// through and for one it has never seen; the reference decides what a frame could see with its rotated pyramid planes (:1329-1367), the
// per-pyramid farthest return and the occlusion rule of mapUpdate (:761), and forgets the answer with the frame.  This layer keeps it:
// one 32-bit stamp per WORLD lattice cell -- the update counter of the last frame whose weight update reached the cell's centre, 0 for
// never -- stored toroidally (cell k of an axis lives in slot k mod n), so that ego motion moves a window over the store instead of
// moving the store.
//
//   k_known_integrate   one lane per cell, a wave = 64 consecutive x of one row (wave-uniform y, z: one toroidal row, wrapped at most once
//                       in x).  The plane tables and the farthest returns go to LDS once per workgroup, which then walks its share of the
//                       rows; pyramid_of (dspmap_device.h) opens with the four outer-plane tests, so a wave wholly outside the wedge leaves
//                       after four dot products.  Only seen lanes store.
//   k_known_clear       the slabs of slots whose lattice cells entered the window since the layer was last synchronised: one launch,
//                       blockIdx.y = axis, up to three slabs (their overlaps are zeroed more than once)
//   k_known_ages        slot order -> the reference's voxel order, stamp -> age, coalesced stores
//   k_known_query       one thread per sample: the age of the cell that holds it
//   k_known_count       the two sums of dspmap_known_stats: a wave reduction and one 64-bit atomic per wave and sum
//   k_known_mask        a wave per 64-bit word of a cast-grid row: ballot of "unknown", then a plain read-OR-write of that word in every
//                       layer (a word belongs to one wave: no atomics)
// Nothing of the map is written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"
#include "dspmap_known_slots.h"   // kn_slot, kn_cell, kn_age

#define KN_TPB 256
#define KN_WAVES (KN_TPB / 64)

__global__ void __launch_bounds__(KN_TPB) k_known_integrate(MapDims d, KnownArgs a, const float* __restrict__ planes_h,
                                                             const float* __restrict__ planes_v, const float* __restrict__ maxlen, int n_items) {
    __shared__ float s_ph[DSP_MAX_PLANES_H * 3];
    __shared__ float s_pv[DSP_MAX_PLANES_V * 3];
    extern __shared__ float s_ml[];   // [np]
    for (int i = threadIdx.x; i < (d.np_h + 1) * 3; i += KN_TPB) s_ph[i] = planes_h[i];
    for (int i = threadIdx.x; i < (d.np_v + 1) * 3; i += KN_TPB) s_pv[i] = planes_v[i];
    for (int i = threadIdx.x; i < d.np; i += KN_TPB) s_ml[i] = maxlen[i];
    __syncthreads();
    const int l = lane_id();
    const int W = (int)grid_row_words(d);
    for (int item = (int)blockIdx.x * KN_WAVES + ((int)threadIdx.x >> 6); item < n_items; item += (int)gridDim.x * KN_WAVES) {
        const int w = item % W, row = item / W, y = row % d.ny, z = row / d.ny;   // (wave-uniform)
        const int x = w * 64 + l;
        const bool in = x < d.nx;
        // the centre of the lattice cell behind voxel (x, y, z), relative to the sensor: two roundings per axis
        const float px = __fadd_rn(__fmul_rn((float)x, d.res), a.ox);
        const float py = __fadd_rn(__fmul_rn((float)y, d.res), a.oy);
        const float pz = __fadd_rn(__fmul_rn((float)z, d.res), a.oz);
        const int b = in ? pyramid_of(d, s_ph, s_pv, px, py, pz) : -1;
        if (!__ballot(b >= 0)) continue;   // the whole wave lies outside the wedge
        if (b < 0) continue;
        const float dist = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(pz, pz)));
        const float ml = s_ml[b];
        const bool occluded = ml > 0.f && dist > __fadd_rn(ml, a.occl_margin);   // :761
        if (!occluded && dist <= a.max_range) a.stamp[kn_cell(d, a, x, y, z)] = a.now;
    }
}

// blockIdx.y = axis; the slab of axis A: slots [s0, s0 + cnt) mod n of that axis, everything of the other two
__global__ void __launch_bounds__(KN_TPB) k_known_clear(MapDims d, unsigned* __restrict__ stamp, int3 s0, int3 cnt) {
    const int ax = blockIdx.y;
    const long long i = (long long)blockIdx.x * KN_TPB + threadIdx.x;
    int x, y, z;
    if (ax == 0) {
        if (cnt.x <= 0 || i >= (long long)cnt.x * d.ny * d.nz) return;
        const int r = (int)(i / cnt.x);
        x = kn_slot((int)(i % cnt.x), s0.x, d.nx); y = r % d.ny; z = r / d.ny;
    } else if (ax == 1) {
        if (cnt.y <= 0 || i >= (long long)cnt.y * d.nx * d.nz) return;
        const int r = (int)(i / d.nx);
        x = (int)(i % d.nx); y = kn_slot(r % cnt.y, s0.y, d.ny); z = r / cnt.y;
    } else {
        if (cnt.z <= 0 || i >= (long long)cnt.z * d.nx * d.ny) return;
        const int r = (int)(i / d.nx);
        x = (int)(i % d.nx); y = r % d.ny; z = kn_slot(r / d.ny, s0.z, d.nz);
    }
    stamp[((size_t)z * d.ny + y) * d.nx + x] = 0u;
}

__global__ void __launch_bounds__(KN_TPB) k_known_ages(MapDims d, KnownArgs a, int* __restrict__ out) {
    const int g = blockIdx.x * KN_TPB + threadIdx.x;
    if (g >= d.v_glob) return;
    const int zc = d.ny * d.nx;
    const int z = g / zc, rest = g - z * zc, y = rest / d.nx, x = rest - y * d.nx;
    out[g] = kn_age(a.stamp[kn_cell(d, a, x, y, z)], a.now);
}

// One thread per sample, as k_dist_query: the cell behind the point's own voxel.  t is not read.
__global__ void __launch_bounds__(KN_TPB) k_known_query(MapDims d, KnownArgs a, SampleOrigin org, int n, const float4* __restrict__ q,
                                                         int* __restrict__ out) {
    const unsigned i = blockIdx.x * KN_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 s = q[i];
    int age = -1;
    if (!(s.x != s.x || s.y != s.y || s.z != s.z)) {
        float px = s.x, py = s.y, pz = s.z;
        origin_apply(org, px, py, pz);
        int g;
        if (voxel_of(d, px, py, pz, g)) {
            const int zc = d.ny * d.nx;
            const int z = g / zc, rest = g - z * zc, y = rest / d.nx, x = rest - y * d.nx;
            age = kn_age(a.stamp[kn_cell(d, a, x, y, z)], a.now);
        }
    }
    out[i] = age;
}

// sums[0] += cells with 0 <= age <= max_age, sums[1] += cells stamped by the current frame (a count over all slots: the window is a
// permutation of them)
__global__ void __launch_bounds__(KN_TPB) k_known_count(MapDims d, KnownArgs a, int max_age, u64* __restrict__ sums) {
    const int g = blockIdx.x * KN_TPB + threadIdx.x;
    const int age = g < d.v_glob ? kn_age(a.stamp[g], a.now) : -1;
    const u64 young = __ballot(age >= 0 && age <= max_age), fresh = __ballot(age == 0);
    if (lane_id() == 0) {
        if (young) atomicAdd(&sums[0], (u64)__popcll(young));
        if (fresh) atomicAdd(&sums[1], (u64)__popcll(fresh));
    }
}

// a wave per word (z, y, w) of a grid row; bits at x >= nx stay 0
__global__ void __launch_bounds__(KN_TPB) k_known_mask(MapDims d, KnownArgs a, int max_age, int L, u64* __restrict__ bits, int n_items) {
    const int item = (int)blockIdx.x * KN_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const int W = (int)grid_row_words(d);
    const int w = item % W, row = item / W, y = row % d.ny, z = row / d.ny;
    const int x = w * 64 + l;
    bool unknown = false;
    if (x < d.nx) {
        const int age = kn_age(a.stamp[kn_cell(d, a, x, y, z)], a.now);
        unknown = age < 0 || age > max_age;
    }
    const u64 word = __ballot(unknown);
    if (!word) return;
    for (int j = l; j < L; j += 64) {   // one lane per layer
        u64* p = bits + (size_t)j * n_items + item;
        *p = *p | word;
    }
}

static unsigned kn_blocks(long long n) { return (unsigned)((n + KN_TPB - 1) / KN_TPB); }
static int kn_words(const MapDims& d) { return (int)grid_layer_words(d); }

void launch_known_integrate(const MapDims& d, const DevState& s, hipStream_t stream, const KnownArgs& a, int n_cu) {
    const int n_items = kn_words(d);
    const int want = (n_items + KN_WAVES - 1) / KN_WAVES, cap = (n_cu > 0 ? n_cu : 256) * 8;   // (a workgroup pays for its tables once)
    hipLaunchKernelGGL(k_known_integrate, dim3((unsigned)(want < cap ? want : cap)), dim3(KN_TPB), sizeof(float) * (size_t)d.np, stream, d, a,
                       s.planes_h, s.planes_v, s.obs_maxlen, n_items);
}
void launch_known_clear(const MapDims& d, hipStream_t stream, unsigned* stamp, const int s0[3], const int cnt[3]) {
    const long long cells[3] = {(long long)cnt[0] * d.ny * d.nz, (long long)cnt[1] * d.nx * d.nz, (long long)cnt[2] * d.nx * d.ny};
    long long most = cells[0] > cells[1] ? cells[0] : cells[1];
    if (cells[2] > most) most = cells[2];
    if (most <= 0) return;
    hipLaunchKernelGGL(k_known_clear, dim3(kn_blocks(most), 3), dim3(KN_TPB), 0, stream, d, stamp, make_int3(s0[0], s0[1], s0[2]),
                       make_int3(cnt[0], cnt[1], cnt[2]));
}
void launch_known_ages(const MapDims& d, hipStream_t stream, const KnownArgs& a, int* out) {
    hipLaunchKernelGGL(k_known_ages, dim3(kn_blocks(d.v_glob)), dim3(KN_TPB), 0, stream, d, a, out);
}
void launch_known_query(const MapDims& d, hipStream_t stream, const KnownArgs& a, const SampleOrigin& org, int n, const float4* q, int* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_known_query, dim3(kn_blocks(n)), dim3(KN_TPB), 0, stream, d, a, org, n, q, out);
}
void launch_known_count(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, u64* sums) {
    hipLaunchKernelGGL(k_known_count, dim3(kn_blocks(d.v_glob)), dim3(KN_TPB), 0, stream, d, a, max_age, sums);
}
void launch_known_mask(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, int L, u64* bits) {
    const int n_items = kn_words(d);
    hipLaunchKernelGGL(k_known_mask, dim3((unsigned)((n_items + KN_WAVES - 1) / KN_WAVES)), dim3(KN_TPB), 0, stream, d, a, max_age, L, bits, n_items);
}
