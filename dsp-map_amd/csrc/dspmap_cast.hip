// dspmap_cast.hip -- segment casts through a bit grid of the current and the predicted occupancy (dspmap_build_cast_grid,
// dspmap_cast_segments*; semantics next to them in include/dspmap.h).  The reference has no counterpart: a planner that asks "is the
// straight segment a -> b free, and where is it blocked first?" copies the whole grid out (getOccupancyMapWithFutureStatus :405-426)
// and walks it on the host.
//
// The grid: one bit per voxel and layer (0: current mass, 1 + k: horizon k) in the reference's voxel order, [L][nz][ny][W] 64-bit words.
//   k_cast_pack        one wave per (row, layer): the masses are read in place and in storage order and balloted into words
//                      (df_row_word, the ballot k_dist_x of dspmap_distance.hip takes its distances from).
//   k_cast_inflate_xy  (r > 0) one lane per word, lanes along the words of a row: OR of the 2r + 1 rows y - r .. y + r of the word and its
//                      two neighbours, then the x dilation as shifts by 1 .. r both ways with the carries out of the neighbouring words
//                      (OR commutes with shifts: one dilation after the ORs).  The pad bits of a row's last word are masked off again.
//   k_cast_inflate_z   (r > 0) one lane per word: OR over the 2r + 1 planes z - r .. z + r.  Nothing is transposed; rows outside the map
//                      contribute nothing, which is the Chebyshev ball clipped at the faces.
//
// The cast: ONE LANE PER SEGMENT, a plain Amanatides-Woo loop per lane -- two 16-byte loads in, one 16-byte store out.  A lane keeps the
// 64-bit word of its current (layer, row, x >> 6) in registers and loads again only when that key changes: steps along x inside a word
// cost no memory access.  The layer of the time a cell is LEFT is carried over as the layer of the time the next one is ENTERED (the two
// are the same fp32 expression of the same parameter), so a space-time cast evaluates k(t) once per cell.
// Divergence of the trip counts between the lanes of a wave is the cost that remains, and the plain loop is the answer chosen here.
// A coarse any-bit-per-4x4x4 grid or a word-level skip along x would have to advance the IDENTICAL fp32 DDA state (tMax += tDelta per
// crossed face, in the same order) through the skipped cells to leave s and the LEFT_MAP cell bit-exact, so a skip saves loads, not
// steps -- and the loads are already rare: the grids are 0.3 MB (66 x 66 x 40, 7 layers) to a few MB and sit in L2, the register word
// covers the x steps, and segments of a planner's batch that start near each other share lines.  What a skip structure adds is a
// second snapshot to build per layer and a second test per step in every lane.  A segment of 3 m at 0.15 m crosses ~20 - 35 cells;
// 131 072 of them are 2 048 waves, eight per CU, whose long lanes overlap other waves' loads.
#include "dspmap_cast_walk.h"
#include "dspmap_internal.h"

#define CAST_TPB 256
#define CAST_WAVES (CAST_TPB / 64)

__global__ void __launch_bounds__(CAST_TPB) k_cast_pack(MapDims d, DevState s, CastGridArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * CAST_WAVES + (threadIdx.x >> 6);   // y + ny * z
    const int layer = blockIdx.y;
    if (row >= d.ny * d.nz) return;   // (wave-uniform: the ballots below see whole waves)
    const int z = row / d.ny, y = row - z * d.ny;
    const int nw = (int)grid_row_words(d);
    u64* out = a.bits + ((size_t)layer * d.ny * d.nz + row) * nw;
    for (int w = 0; w < nw; ++w) {
        const u64 word = df_row_word(d, s, a.thr, a.fut_zero, layer, w * 64 + lane, y, z);
        if (lane == 0) out[w] = word;
    }
}

// bits -> tmp: OR over the rows y - r .. y + r of the same plane, dilated by r along x
__global__ void __launch_bounds__(CAST_TPB) k_cast_inflate_xy(MapDims d, CastGridArgs a, unsigned n_words) {
    const unsigned t = blockIdx.x * CAST_TPB + threadIdx.x;
    if (t >= n_words) return;
    const unsigned nw = grid_row_words(d);
    const unsigned w = t % nw, row = t / nw;          // row = y + ny * (z + nz * layer)
    const int y = (int)(row % (unsigned)d.ny);
    const int y0 = max(y - a.r, 0), y1 = min(y + a.r, d.ny - 1);
    u64 c = 0, p = 0, q = 0;                          // the word, the one below it along x, the one above
    for (int yy = y0; yy <= y1; ++yy) {
        const u64* in = a.bits + ((size_t)row - y + yy) * nw + w;
        c |= in[0];
        if (w > 0) p |= in[-1];
        if (w + 1 < nw) q |= in[1];
    }
    u64 o = c;
    for (int sft = 1; sft <= a.r; ++sft) o |= (c << sft) | (c >> sft) | (p >> (64 - sft)) | (q << (64 - sft));
    if (w + 1 == nw) o &= grid_row_mask(d);           // bits at x >= nx stay 0
    a.tmp[t] = o;
}

// tmp -> bits: OR over the planes z - r .. z + r of the same layer
__global__ void __launch_bounds__(CAST_TPB) k_cast_inflate_z(MapDims d, CastGridArgs a, unsigned n_words) {
    const unsigned t = blockIdx.x * CAST_TPB + threadIdx.x;
    if (t >= n_words) return;
    const unsigned plane = GridWords(d).plane;
    const int z = (int)((t / plane) % (unsigned)d.nz);
    const int z0 = max(z - a.r, 0), z1 = min(z + a.r, d.nz - 1);
    u64 o = 0;
    for (int zz = z0; zz <= z1; ++zz) o |= a.tmp[(long long)t + (long long)(zz - z) * (long long)plane];
    a.bits[t] = o;
}

__global__ void __launch_bounds__(CAST_TPB) k_cast(MapDims d, CastArgs a, int n, const float4* __restrict__ seg, int4* __restrict__ out) {
    const unsigned i = blockIdx.x * CAST_TPB + threadIdx.x;   // (unsigned: n may come within a block of INT_MAX)
    if (i >= (unsigned)n) return;
    const float4 A = seg[2 * (size_t)i], B = seg[2 * (size_t)i + 1];   // {ax, ay, az, ta}, {bx, by, bz, tb}
    float s = 0.f;
    int voxel = -1, layer = -1, status = DSPMAP_CAST_INVALID;
    const bool valid = grid_finite(A.x) && grid_finite(A.y) && grid_finite(A.z) && grid_finite(B.x) && grid_finite(B.y) && grid_finite(B.z) &&
                       A.w == A.w && B.w == B.w;
    if (valid) {
        float ax = A.x, ay = A.y, az = A.z, bx = B.x, by = B.y, bz = B.z;
        origin_apply(a.org, ax, ay, az, bx, by, bz);
        cast_walk(d, a.bits, ax, ay, az, A.w, bx, by, bz, B.w, s, voxel, layer, status);
    }
    out[i] = make_int4(__float_as_int(s), voxel, layer, status);
}

void launch_cast_grid(const LaunchCtx& c, const CastGridArgs& a) {
    const MapDims& d = c.d;
    const int rows = d.ny * d.nz;
    hipLaunchKernelGGL(k_cast_pack, dim3((rows + CAST_WAVES - 1) / CAST_WAVES, a.L), dim3(CAST_TPB), 0, c.stream, d, c.s, a);
    if (a.r <= 0) return;
    const unsigned n_words = (unsigned)((size_t)a.L * grid_layer_words(d));   // (< 2^31: dspmap_build_cast_grid refuses more)
    const dim3 g((n_words + CAST_TPB - 1) / CAST_TPB);
    hipLaunchKernelGGL(k_cast_inflate_xy, g, dim3(CAST_TPB), 0, c.stream, d, a, n_words);
    hipLaunchKernelGGL(k_cast_inflate_z, g, dim3(CAST_TPB), 0, c.stream, d, a, n_words);
}

void launch_cast(const LaunchCtx& c, const CastArgs& a, int n, const dspmap_segment* seg, dspmap_cast_hit* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cast, dim3((unsigned)(((long long)n + CAST_TPB - 1) / CAST_TPB)), dim3(CAST_TPB), 0, c.stream, c.d, a, n,
                       (const float4*)seg, (int4*)out);
}
