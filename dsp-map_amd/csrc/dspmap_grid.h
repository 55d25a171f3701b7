// dspmap_grid.h -- what the planning kernels share about the map's lattice and about the cast grid's bit sets, each rule ONCE:
//   the cell of a sample   grid_finite, origin_apply, grid_axis_cell, grid_cell (include/dspmap.h: the rules of the queries and of cast step 2)
//   the word layout        GridWords, grid_row_words, grid_layer_words: [L][nz][ny][W] 64-bit words, W = ceil(nx / 64), bit = x & 63
//   the wavefronts' parts  grid_grow6, grid_store_bits (k_reach of dspmap_reach.hip, k_cost_wave of dspmap_cost.hip)
// Every device helper performs exactly the operations it was lifted from, in their order and with the explicit __f*_rn intrinsics: the
// results are compared bit for bit with host references that round every operation once.
//
// Out of scope: voxel_of and div_res of dspmap_device.h.  The filter and the query kernels that call them take the verified reciprocal
// path (MapDims::div_ok) and keep it.  Both rules put a point in the same cell, because both truncate the CORRECTLY ROUNDED fp32 quotient
// (p + half) / res: __fdiv_rn is the IEEE division, and div_res's three operations are used only where a kernel has shown them equal to it.
#pragma once
#include <hip/hip_runtime.h>

#include "dspmap_kernels.h"   // SampleOrigin
#include "dspmap_types.h"

// ---- the word layout.  Two forms, one per kind of site: the free functions for a site that needs W or a layer's size in its own integer type
// (the host sizes its buffers with them), GridWords for the wave kernels, whose every index is 32-bit unsigned
__host__ __device__ __forceinline__ unsigned grid_row_words(const MapDims& d) { return (unsigned)(d.nx + 63) >> 6; }   // W
__host__ __device__ __forceinline__ size_t grid_layer_words(const MapDims& d) { return (size_t)d.nz * d.ny * grid_row_words(d); }
// the mask of a row's last word: bits at x >= nx are never set
__host__ __device__ __forceinline__ u64 grid_row_mask(const MapDims& d) { return (d.nx & 63) ? ~0ull >> (64 - (d.nx & 63)) : ~0ull; }
struct GridWords {
    unsigned W, plane, nwords;   // words of a row, of a z plane and of a layer (< 2^31: the cast grid exists)
    __device__ __forceinline__ explicit GridWords(const MapDims& d) : W(grid_row_words(d)), plane((unsigned)d.ny * W), nwords((unsigned)d.nz * plane) {}
    __device__ __forceinline__ unsigned word_of(const MapDims& d, int x, int y, int z) const { return ((unsigned)z * d.ny + y) * W + ((unsigned)x >> 6); }
    __device__ static __forceinline__ u64 bit_of(int x) { return 1ull << (x & 63); }
};

// ---- the cell of a sample
__device__ __forceinline__ bool grid_finite(float v) { return fabsf(v) < INFINITY; }   // (false for NaN)
__device__ __forceinline__ int grid_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// a sample's coordinates in the map frame: minus the sensor position when the caller's are in the world frame
__device__ __forceinline__ void origin_apply(const SampleOrigin& o, float& x, float& y, float& z) {
    if (o.world) { x = __fsub_rn(x, o.ox); y = __fsub_rn(y, o.oy); z = __fsub_rn(z, o.oz); }
}
// ... and both ends of a segment.  This overload exists for one reason only: ONE test of `world` around the six subtractions, which two
// calls of the one above do not give (k_cast, k_grow_boxes)
__device__ __forceinline__ void origin_apply(const SampleOrigin& o, float& ax, float& ay, float& az, float& bx, float& by, float& bz) {
    if (o.world) {
        ax = __fsub_rn(ax, o.ox); ay = __fsub_rn(ay, o.oy); az = __fsub_rn(az, o.oz);
        bx = __fsub_rn(bx, o.ox); by = __fsub_rn(by, o.oy); bz = __fsub_rn(bz, o.oz);
    }
}
// the cell index along one axis of a coordinate inside the map (>= 0: p > -half)
__device__ __forceinline__ int grid_axis_cell(float p, float half, float res) { return (int)__fdiv_rn(__fadd_rn(p, half), res); }
// dspmap_point_voxel_index's test, for NaN-free coordinates
__device__ __forceinline__ bool grid_beyond(const MapDims& d, float px, float py, float pz) {
    return fabsf(px) >= d.half_x || fabsf(py) >= d.half_y || fabsf(pz) >= d.half_z;
}
// the cell of a source / start point: 0 = a cell, -2 = outside the map, -3 = a non-finite coordinate.  The whole rule in one body: the
// finite test, origin_apply's subtraction, grid_beyond's test, grid_axis_cell per axis, the far faces
__device__ __forceinline__ int grid_cell(const MapDims& d, const SampleOrigin o, float px, float py, float pz, int& x, int& y, int& z) {
    if (!(grid_finite(px) && grid_finite(py) && grid_finite(pz))) return -3;
    if (o.world) { px = __fsub_rn(px, o.ox); py = __fsub_rn(py, o.oy); pz = __fsub_rn(pz, o.oz); }
    if (fabsf(px) >= d.half_x || fabsf(py) >= d.half_y || fabsf(pz) >= d.half_z) return -2;   // dspmap_point_voxel_index's test
    x = grid_axis_cell(px, d.half_x, d.res);
    y = grid_axis_cell(py, d.half_y, d.res);
    z = grid_axis_cell(pz, d.half_z, d.res);
    return (x < d.nx && y < d.ny && z < d.nz) ? 0 : -2;
}

// ---- the parts of a one-workgroup-per-field wavefront over bit sets in the word layout (k_reach, k_cost_wave).  The seeding loop and the
// three-flag vote around the single barrier per step stay written out in both kernels, over grid_cell and GridWords: a kernel's step
// loop is held to the instructions it had

// The six face neighbours of the cells of word c = cur[0] (read once, by the caller), word w of row (y, z): its two shifts, the carries
// of the row's neighbouring words (never across rows), the words at y +- 1 and z +- 1.  Six more reads; bits at x >= nx may be set.
// SELF: the word itself is part of the result (k_reach), ORed in first: c | c << 1 | c >> 1 is one three-input OR per half
template <bool SELF>
__device__ __forceinline__ u64 grid_grow6(const u64* cur, u64 c, unsigned w, unsigned y, unsigned z, const GridWords& gw, const MapDims& d) {
    u64 g = (SELF ? c : 0ull) | (c << 1) | (c >> 1);
    if (w > 0) g |= cur[-1] >> 63;
    if (w + 1 < gw.W) g |= cur[1] << 63;
    if (y > 0) g |= cur[-(int)gw.W];
    if (y + 1 < (unsigned)d.ny) g |= cur[gw.W];
    if (z > 0) g |= cur[-(int)gw.plane];
    if (z + 1 < (unsigned)d.nz) g |= cur[gw.plane];
    return g;
}
// the cells of a word's set bits get `value`: cell = the field's entry of the word's bit 0.  FIRST: only where the entry still reads
// `unset` (k_reach: a cell that comes back keeps its first arrival).  The owner of a word is the only thread that touches its 64 entries.
template <bool FIRST = false>
__device__ __forceinline__ void grid_store_bits(unsigned short* cell, u64 bits, unsigned short value, unsigned short unset = 0) {
    while (bits) {
        const int bit = __builtin_ctzll(bits);
        bits &= bits - 1;
        if (!FIRST || cell[bit] == unset) cell[bit] = value;
    }
}
