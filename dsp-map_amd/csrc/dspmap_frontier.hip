// dspmap_frontier.hip -- frontier cells and frontier blocks between known-free and unknown space (dspmap_build_frontiers and its accessors;
// semantics next to them in include/dspmap.h).  The reference has no counterpart.  Inputs: one layer of the cast grid as it is and the
// synchronised known-space layer; everything is an integer predicate, so the outputs are defined bit for bit.
//
//   k_frontier_mark    one wave per word item (z, y, w) of a grid row, lane = x (the shape of k_known_mask; y, z wave-uniform).  A lane reads
//                      its own stamp and those of the rows y -+ 1, z -+ 1 (toroidal slots per axis; a row outside the map contributes
//                      nothing).  The x neighbours come from the wave's own ballot of "unknown", shifted by one; the edge cells of the
//                      neighbouring words (x0 - 1 >= 0, x0 + 64 < nx) are two wave-uniform loads.  One lane stores the frontier word and the
//                      item's count of free cells.  The frontier lanes of a wave that share a block are a run of consecutive lanes: their
//                      count, index sums and sum of u are popcounts of ballots under the run's mask (the sum of lane numbers and of u by bit
//                      planes), and the run's first frontier lane adds them to the block's accumulator: five integer atomics per (wave,
//                      block) that holds a frontier cell, none elsewhere.  Integer sums do not depend on the order of arrival.
//   k_frontier_sums    ordered compaction, step 1: a workgroup per tile of FR_TILE items sums the popcounts of its frontier words (and its
//                      free counts); behind the cell tiles, the block tiles count their non-empty accumulators.
//   k_frontier_scan    step 2: ONE workgroup per list (cells, blocks) turns the tile sums into exclusive bases, chunk by chunk with a carry,
//                      and writes the counts {n_cells, n_blocks, n_free}.
//   k_frontier_emit    step 3: a tile scans its own items again; for the cells each wave walks its 64 items and a lane writes voxel
//                      (row, x0 + lane) at base + popcount(word & lanes below); for the blocks a thread writes its record at base + rank.
//                      Items, bits and blocks are visited in ascending order, so the lists are ascending whatever the launch.
// No kernel waits for another workgroup: the three steps are three launches.  Nothing of the map, the grid or the layer is written.
#include "dspmap_grid.h"
#include "dspmap_internal.h"
#include "dspmap_block_scan.h"    // block_incl_scan_i
#include "dspmap_known_slots.h"   // kn_cell, kn_age

#define FR_TPB 256
#define FR_WAVES (FR_TPB / 64)
static_assert(FR_TILE == FR_TPB, "a tile is one item per thread");

__device__ __forceinline__ bool fr_unknown(const MapDims& d, const FrontierArgs& a, int x, int y, int z) {
    const int age = kn_age(a.kn.stamp[kn_cell(d, a.kn, x, y, z)], a.kn.now);
    return age < 0 || age > a.max_age;
}

template <bool MERGE>
__global__ void __launch_bounds__(FR_TPB) k_frontier_mark(MapDims d, FrontierArgs a, int n_items) {
    const int item = (int)blockIdx.x * FR_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const int W = (int)grid_row_words(d);
    const int w = item % W, row = item / W, y = row % d.ny, z = row / d.ny;
    const int x0 = w * 64, x = x0 + l;
    const bool in = x < d.nx;
    bool unk = false;
    int u = 0;
    if (in) {
        unk = fr_unknown(d, a, x, y, z);
        if (y > 0) u += fr_unknown(d, a, x, y - 1, z) ? 1 : 0;
        if (y + 1 < d.ny) u += fr_unknown(d, a, x, y + 1, z) ? 1 : 0;
        if (z > 0) u += fr_unknown(d, a, x, y, z - 1) ? 1 : 0;
        if (z + 1 < d.nz) u += fr_unknown(d, a, x, y, z + 1) ? 1 : 0;
    }
    const u64 ub = __ballot(unk);   // (lanes at x >= nx give 0: the outside of the map does not exist)
    const bool edge_lo = x0 > 0 && fr_unknown(d, a, x0 - 1, y, z);          // (wave-uniform)
    const bool edge_hi = x0 + 64 < d.nx && fr_unknown(d, a, x0 + 64, y, z);
    const u64 below = (ub << 1) | (edge_lo ? 1ull : 0ull), above = (ub >> 1) | (edge_hi ? 1ull << 63 : 0ull);
    u += (int)((below >> l) & 1ull) + (int)((above >> l) & 1ull);
    const bool fre = in && !unk && !((a.bits[item] >> l) & 1ull);
    const bool fr = fre && u >= a.min_unknown;
    const u64 fw = __ballot(fr), freew = __ballot(fre);
    if (l == 0) {
        a.grid[item] = fw;
        a.item_free[item] = (int)__popcll(freew);
    }
    if (!fw) return;   // (wave-uniform)
    const int X = x / a.block;
    dspmap_frontier_block* b = a.dense + ((size_t)(z / a.block) * a.nby + y / a.block) * a.nbx + X;
    if (!MERGE) {   // DSPMAP_P_FRONTIER_MERGE = 0: every frontier lane adds its own cell
        if (fr) {
            atomicAdd(&b->count, 1);
            atomicAdd(&b->sum_x, x);
            atomicAdd(&b->sum_y, y);
            atomicAdd(&b->sum_z, z);
            atomicAdd(&b->unknown_faces, u);
        }
        return;
    }
    // ---- the wave's share of the block sums: the lanes of block X are the run [X * block, (X + 1) * block) clipped to the word
    const u64 u0 = __ballot(fr && (u & 1)), u1 = __ballot(fr && (u & 2)), u2 = __ballot(fr && (u & 4));
    int lo = X * a.block - x0, hi = lo + a.block;
    if (lo < 0) lo = 0;
    if (hi > 64) hi = 64;
    const u64 m = fw & ((hi - lo >= 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo);
    if (!fr || (m & lanemask_lt())) return;   // the run's first frontier lane goes on
    const int cnt = (int)__popcll(m);
    const int lanes = (int)__popcll(m & 0xaaaaaaaaaaaaaaaaull) + 2 * (int)__popcll(m & 0xccccccccccccccccull) +
                      4 * (int)__popcll(m & 0xf0f0f0f0f0f0f0f0ull) + 8 * (int)__popcll(m & 0xff00ff00ff00ff00ull) +
                      16 * (int)__popcll(m & 0xffff0000ffff0000ull) + 32 * (int)__popcll(m & 0xffffffff00000000ull);
    const int faces = (int)__popcll(m & u0) + 2 * (int)__popcll(m & u1) + 4 * (int)__popcll(m & u2);
    atomicAdd(&b->count, cnt);
    atomicAdd(&b->sum_x, x0 * cnt + lanes);
    atomicAdd(&b->sum_y, y * cnt);
    atomicAdd(&b->sum_z, z * cnt);
    atomicAdd(&b->unknown_faces, faces);
}

// what thread `tid` of tile `tile` counts: the cells of its frontier word (tiles [0, ntc)) or its block being non-empty (tiles behind)
__device__ __forceinline__ int fr_item_count(const FrontierArgs& a, int n_items, int ntc, int tile, int tid) {
    if (tile < ntc) {
        const long long i = (long long)tile * FR_TILE + tid;
        return i < n_items ? (int)__popcll(a.grid[i]) : 0;
    }
    const long long i = (long long)(tile - ntc) * FR_TILE + tid;
    return i < a.nb && a.dense[i].count > 0 ? 1 : 0;
}

__global__ void __launch_bounds__(FR_TPB) k_frontier_sums(FrontierArgs a, int n_items, int ntc) {
    __shared__ int s_w[FR_WAVES];
    const int tile = (int)blockIdx.x;
    int total;
    (void)block_incl_scan_i<FR_WAVES>(fr_item_count(a, n_items, ntc, tile, (int)threadIdx.x), s_w, total);
    if (threadIdx.x == 0) a.tile_sum[tile] = total;
    if (tile < ntc) {
        const long long i = (long long)tile * FR_TILE + threadIdx.x;
        (void)block_incl_scan_i<FR_WAVES>(i < n_items ? a.item_free[i] : 0, s_w, total);
        if (threadIdx.x == 0) a.tile_free[tile] = total;
    }
}

// blockIdx.x = 0: the cell tiles [0, ntc) -> counts[0], and their free cells -> counts[2]; 1: the block tiles [ntc, ntc + ntb) -> counts[1]
__global__ void __launch_bounds__(FR_TPB) k_frontier_scan(FrontierArgs a, int ntc, int ntb) {
    __shared__ int s_w[FR_WAVES];
    __shared__ long long s_free[FR_WAVES];
    const bool cells = blockIdx.x == 0;
    int* t = a.tile_sum + (cells ? 0 : ntc);
    const int n = cells ? ntc : ntb;
    long long carry = 0, fre = 0;
    for (int base = 0; base < n; base += FR_TPB) {   // (uniform trip count)
        const int i = base + (int)threadIdx.x;
        const int v = i < n ? t[i] : 0;
        int total;
        const int inc = block_incl_scan_i<FR_WAVES>(v, s_w, total);
        if (i < n) {
            t[i] = (int)carry + inc - v;   // (n_cells <= V < 2^31)
            if (cells) fre += a.tile_free[i];
        }
        carry += total;
    }
    if (cells) {   // n_free: lanes -> wave -> workgroup, in 64 bits all the way
        for (int o = 32; o > 0; o >>= 1) fre += __shfl_xor(fre, o, WAVE);
        if (lane_id() == 0) s_free[threadIdx.x >> 6] = fre;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long f = 0;
            for (int j = 0; j < FR_WAVES; ++j) f += s_free[j];
            a.counts[2] = f;
        }
    }
    if (threadIdx.x == 0) a.counts[cells ? 0 : 1] = carry;
}

__global__ void __launch_bounds__(FR_TPB) k_frontier_emit(MapDims d, FrontierArgs a, int n_items, int ntc) {
    __shared__ int s_w[FR_WAVES];
    __shared__ int s_base[FR_TILE];
    const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int c = fr_item_count(a, n_items, ntc, tile, tid);
    int total;
    const int at = a.tile_sum[tile] + block_incl_scan_i<FR_WAVES>(c, s_w, total) - c;   // where this thread's item starts in its list
    if (tile >= ntc) {   // (workgroup-uniform) a block record
        if (c) {
            const int i = (tile - ntc) * FR_TILE + tid;
            dspmap_frontier_block r = a.dense[i];
            r.block = i;
            a.blocks[at] = r;
        }
        return;
    }
    s_base[tid] = at;
    __syncthreads();
    const int l = lane_id(), wv = tid >> 6;
    const int W = (int)grid_row_words(d);
    for (int k = 0; k < 64; ++k) {
        const long long item = (long long)tile * FR_TILE + wv * 64 + k;
        if (item >= n_items) break;   // (wave-uniform)
        const u64 word = a.grid[item];
        if (!word) continue;
        if ((word >> l) & 1ull) {
            const int w = (int)(item % W), row = (int)(item / W);
            a.cells[s_base[wv * 64 + k] + (int)__popcll(word & lanemask_lt())] = row * d.nx + w * 64 + l;
        }
    }
}

void launch_frontiers(const MapDims& d, hipStream_t stream, const FrontierArgs& a) {
    const int n_items = (int)grid_layer_words(d);
    const int ntc = frontier_tiles(n_items), ntb = frontier_tiles(a.nb);
    const dim3 grid((unsigned)((n_items + FR_WAVES - 1) / FR_WAVES));
    if (a.merge) hipLaunchKernelGGL(k_frontier_mark<true>, grid, dim3(FR_TPB), 0, stream, d, a, n_items);
    else hipLaunchKernelGGL(k_frontier_mark<false>, grid, dim3(FR_TPB), 0, stream, d, a, n_items);
    hipLaunchKernelGGL(k_frontier_sums, dim3((unsigned)(ntc + ntb)), dim3(FR_TPB), 0, stream, a, n_items, ntc);
    hipLaunchKernelGGL(k_frontier_scan, dim3(2), dim3(FR_TPB), 0, stream, a, ntc, ntb);
    hipLaunchKernelGGL(k_frontier_emit, dim3((unsigned)(ntc + ntb)), dim3(FR_TPB), 0, stream, d, a, n_items, ntc);
}
