// dspmap_objects.hip -- the connected components of one layer of the cast grid as objects: box, index sums, fixed-point mass and momentum
// (dspmap_build_objects and its accessors; semantics next to them in include/dspmap.h).  The reference has no counterpart.  Inputs: one
// layer of the cast grid as it is and the current result grid; every output is an integer, so the build is defined bit for bit.
//
// Union-find on labels that only ever decrease (dspmap_unionfind.h, where the termination argument stands), in separate launches:
//   k_objects_init     one wave per word item (z, y, w) of a grid row, lane = x.  A set cell's label is the voxel index of the first cell of
//                      its run of consecutive set bits in the word: bit operations on the word, so x-adjacency inside a word costs nothing.
//                      A clear cell gets -1.
//   k_objects_merge    one wave per word item.  The word is ANDed with the words of the lower half of the neighbourhood -- the previous
//                      word's last bit (x - 1 across the word edge), the rows (y - 1, z) and (y, z - 1), and for 26 also (y - 1, z - 1) and
//                      (y + 1, z - 1) and every row shifted by one in x either way (the ten diagonals).  Consecutive bits of such an AND
//                      join the same two runs, so only the first lane of each of its runs unites; and a diagonal counts only where it is
//                      the sole contact (neither cell between the two is set), since otherwise the straight unions join them already.
//   k_objects_flatten  L[v] = find(v): roots do not change in this launch, and a root is the smallest voxel index of its component.
//   k_objects_count    cells per root: the first lane of every run adds the run's length.
//   k_objects_sums / _scan / _emit   ordered compaction (the pattern of dspmap_frontier.hip) of the roots with count >= min_cells into
//                      ordinals, ascending; _sums also counts the roots and the set cells; _emit replaces a root's count by its ordinal
//                      (-1 below min_cells) and starts the records of the ordinals below max_objects.
//   k_objects_accumulate   one wave per word item: every cell's ordinal into the label grid; per run -- per word where all its runs belong
//                      to one object -- the box by integer atomicMin / atomicMax behind a plain look (bounds only move outwards), the
//                      index sums by popcounts and the two fixed-point sums (a wave prefix sum, then the difference over the run) by
//                      64-bit integer atomicAdd.  Integer sums do not depend on the order of arrival.
// No kernel waits for another workgroup, there is no cooperative launch and no host read between the launches.  A find or unite that
// meets a broken invariant or runs out of its trip bound ORs its code into the counts buffer's fault word and goes on; the synchronous
// accessors turn a non-zero word into an error.  Nothing of the map or the grid is written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"
#include "dspmap_block_scan.h"
#include "dspmap_unionfind.h"

#define OB_TPB 256
#define OB_WAVES (OB_TPB / 64)
static_assert(FR_TILE == OB_TPB, "a tile is one voxel per thread");
static_assert(sizeof(dspmap_object) == 88, "dspmap_object is 88 bytes");

// the label array as uf_find / uf_unite see it: loads at agent scope (another workgroup's atomicMin is seen, not this CU's cached line)
struct ObLabels {
    int* L;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int atomic_min(int i, int v) const { return atomicMin(L + i, v); }
};

// word item -> (w, y, z); row = z * ny + y
struct ObItem { int w, row, y, z, x0; };
__device__ __forceinline__ ObItem ob_item(const MapDims& d, int item) {
    const int W = (int)grid_row_words(d);
    ObItem it;
    it.w = item % W; it.row = item / W; it.y = it.row % d.ny; it.z = it.row / d.ny; it.x0 = it.w * 64;
    return it;
}
// word w of a row, its bits at x >= nx cleared (the grid keeps them clear; the labels' indices must not depend on that)
__device__ __forceinline__ u64 ob_word(const MapDims& d, const u64* __restrict__ bits, int item, int w) {
    const int left = d.nx - w * 64;
    return bits[item] & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
}
// length of the run of set bits of `word` that starts at bit l (bit l is set)
__device__ __forceinline__ int ob_run_len(u64 word, int l) {
    const u64 t = ~(word >> l);
    return t ? (int)__ffsll((long long)t) - 1 : 64 - l;   // (t == 0: l == 0 and the word is full)
}
// the sum of the lane numbers of the bits of m, by bit planes
__device__ __forceinline__ int ob_lane_sum(u64 m) {
    return (int)__popcll(m & 0xaaaaaaaaaaaaaaaaull) + 2 * (int)__popcll(m & 0xccccccccccccccccull) + 4 * (int)__popcll(m & 0xf0f0f0f0f0f0f0f0ull) +
           8 * (int)__popcll(m & 0xff00ff00ff00ff00ull) + 16 * (int)__popcll(m & 0xffff0000ffff0000ull) + 32 * (int)__popcll(m & 0xffffffff00000000ull);
}
__device__ __forceinline__ void ob_fault(const ObjectArgs& a, int fault) {
    if (fault) atomicOr((unsigned long long*)&a.counts[3], (unsigned long long)fault);
}

__global__ void __launch_bounds__(OB_TPB) k_objects_init(MapDims d, ObjectArgs a, int n_items) {
    const int item = (int)blockIdx.x * OB_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const ObItem it = ob_item(d, item);
    const int x = it.x0 + l;
    if (x >= d.nx) return;
    const u64 word = ob_word(d, a.bits, item, it.w);
    int lab = -1;
    if ((word >> l) & 1ull) {
        const u64 starts = word & ~(word << 1);                  // the first bit of every run
        const u64 upto = starts & (~0ull >> (63 - l));           // ... at or below this lane: not empty
        lab = it.row * d.nx + it.x0 + 63 - (int)__clzll((long long)upto);
    }
    a.parent[it.row * d.nx + x] = lab;
}

template <bool C26>
__global__ void __launch_bounds__(OB_TPB) k_objects_merge(MapDims d, ObjectArgs a, int n_items) {
    const int item = (int)blockIdx.x * OB_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const ObItem it = ob_item(d, item);
    const u64 word = ob_word(d, a.bits, item, it.w);
    if (!word) return;             // (wave-uniform)
    const int W = (int)grid_row_words(d), V = d.v_glob;
    ObLabels m{a.parent};
    const int g = it.row * d.nx + it.x0 + l;
    int fault = UF_OK;
    // every lane whose bit is set in `mine` has a set neighbour at voxel index ng: consecutive bits join the same two runs, so the first
    // one of each run of bits unites
    auto unite_first = [&](u64 mine, int ng) {
        const u64 first = mine & ~(mine << 1);
        if ((first >> l) & 1ull) fault |= uf_unite(m, g, ng, V);
    };
    const u64 own_lo = it.w > 0 ? ob_word(d, a.bits, item - 1, it.w - 1) >> 63 : 0ull;          // this row's cells at x0 - 1 and x0 + 64
    const u64 own_hi = it.w + 1 < W ? ob_word(d, a.bits, item + 1, it.w + 1) & 1ull : 0ull;
    if (own_lo) unite_first(word & 1ull, g - 1);   // x - 1 across the word edge
    auto row = [&](int dy, int dz) {
        const int yy = it.y + dy, zz = it.z + dz;
        if (yy < 0 || yy >= d.ny || zz < 0) return;   // (wave-uniform) outside the map: does not exist
        const int nrow = zz * d.ny + yy, nitem = nrow * W + it.w;
        const u64 nb = ob_word(d, a.bits, nitem, it.w);
        const int ng = nrow * d.nx + it.x0 + l;
        unite_first(word & nb, ng);
        if (C26) {
            // a diagonal neighbour counts only where it is the sole contact: with the cell between them set in either row, the two are
            // joined through it (x-adjacent cells of a row are one run; the cell's own union with the other row is the line above, in
            // this wave or in the neighbouring word's)
            const u64 lo = it.w > 0 ? ob_word(d, a.bits, nitem - 1, it.w - 1) >> 63 : 0ull;
            const u64 hi = it.w + 1 < W ? ob_word(d, a.bits, nitem + 1, it.w + 1) & 1ull : 0ull;
            unite_first(word & ((nb << 1) | lo) & ~nb & ~((word << 1) | own_lo), ng - 1);
            unite_first(word & ((nb >> 1) | (hi << 63)) & ~nb & ~((word >> 1) | (own_hi << 63)), ng + 1);
        }
    };
    row(-1, 0);
    row(0, -1);
    if (C26) {
        row(-1, -1);
        row(1, -1);
    }
    ob_fault(a, fault);
}

__global__ void __launch_bounds__(OB_TPB) k_objects_flatten(MapDims d, ObjectArgs a) {
    const int v = (int)(blockIdx.x * OB_TPB + threadIdx.x);
    if (v >= d.v_glob) return;
    ObLabels m{a.parent};
    const int p = m.load(v);
    if (p < 0 || p == v) return;   // clear, or a root already
    int fault = UF_OK;
    const int r = uf_find(m, p, d.v_glob, &fault);
    if (r >= 0) a.parent[v] = r;
    ob_fault(a, fault);
}

__global__ void __launch_bounds__(OB_TPB) k_objects_count(MapDims d, ObjectArgs a, int n_items) {
    const int item = (int)blockIdx.x * OB_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const ObItem it = ob_item(d, item);
    const u64 word = ob_word(d, a.bits, item, it.w);
    const u64 starts = word & ~(word << 1);
    if (!((starts >> l) & 1ull)) return;
    const int r = a.parent[it.row * d.nx + it.x0 + l];
    if (r >= 0) atomicAdd(&a.root_val[r], ob_run_len(word, l));   // (r < 0: a fault has been recorded)
}

// thread `tid` of tile `tile`: is its voxel a root (root: its count, else -1)
__device__ __forceinline__ int ob_root_count(const MapDims& d, const ObjectArgs& a, long long i, int& p) {
    p = i < d.v_glob ? a.parent[i] : -1;
    return p == (int)i ? a.root_val[i] : -1;
}

__global__ void __launch_bounds__(OB_TPB) k_objects_sums(MapDims d, ObjectArgs a) {
    __shared__ int s_w[OB_WAVES];
    const int tile = (int)blockIdx.x;
    int p, total, roots, occ;
    const int c = ob_root_count(d, a, (long long)tile * FR_TILE + threadIdx.x, p);
    (void)block_incl_scan_i<OB_WAVES>(c >= a.min_cells ? 1 : 0, s_w, total);
    (void)block_incl_scan_i<OB_WAVES>(c >= 0 ? 1 : 0, s_w, roots);
    (void)block_incl_scan_i<OB_WAVES>(p >= 0 ? 1 : 0, s_w, occ);
    if (threadIdx.x == 0) {
        a.tile_sum[tile] = total;
        if (roots) atomicAdd((unsigned long long*)&a.counts[1], (unsigned long long)roots);
        if (occ) atomicAdd((unsigned long long*)&a.counts[2], (unsigned long long)occ);
    }
}

// ONE workgroup: the tile sums -> exclusive bases, chunk by chunk with a carry; counts[0]
__global__ void __launch_bounds__(OB_TPB) k_objects_scan(ObjectArgs a, int n_tiles) {
    __shared__ int s_w[OB_WAVES];
    long long carry = 0;
    for (int base = 0; base < n_tiles; base += OB_TPB) {   // (uniform trip count)
        const int i = base + (int)threadIdx.x;
        const int v = i < n_tiles ? a.tile_sum[i] : 0;
        int total;
        const int inc = block_incl_scan_i<OB_WAVES>(v, s_w, total);
        if (i < n_tiles) a.tile_sum[i] = (int)carry + inc - v;   // (n_objects <= V < 2^31)
        carry += total;
    }
    if (threadIdx.x == 0) a.counts[0] = carry;
}

__global__ void __launch_bounds__(OB_TPB) k_objects_emit(MapDims d, ObjectArgs a) {
    __shared__ int s_w[OB_WAVES];
    const int tile = (int)blockIdx.x;
    const long long i = (long long)tile * FR_TILE + threadIdx.x;
    int p, total;
    const int c = ob_root_count(d, a, i, p);
    const int sel = c >= a.min_cells ? 1 : 0;   // (min_cells >= 1 > -1)
    const int at = a.tile_sum[tile] + block_incl_scan_i<OB_WAVES>(sel, s_w, total) - sel;
    if (c < 0) return;   // not a root
    a.root_val[i] = sel ? at : -1;   // (only this thread reads or writes the entry in this launch)
    if (sel && at < a.max_objects) {
        dspmap_object o;
        o.label = (int)i; o.count = c;
        o.min_x = o.min_y = o.min_z = 0x7fffffff;
        o.max_x = o.max_y = o.max_z = -1;
        o.sum_x = o.sum_y = o.sum_z = 0; o.mass_q = 0; o.mom_q[0] = o.mom_q[1] = o.mom_q[2] = 0;
        a.objects[at] = o;
    }
}

__device__ __forceinline__ void ob_add64(long long* p, long long v) {
    if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}
// x * 2^20 as a truncated integer: the product is exact for |x| < 4096
__device__ __forceinline__ long long ob_q20(float x) { return (long long)__fmul_rn(x, 1048576.0f); }

__global__ void __launch_bounds__(OB_TPB) k_objects_accumulate(MapDims d, DevState s, ObjectArgs a, int n_items) {
    const int item = (int)blockIdx.x * OB_WAVES + ((int)threadIdx.x >> 6);
    if (item >= n_items) return;   // (wave-uniform)
    const int l = lane_id();
    const ObItem it = ob_item(d, item);
    const u64 word = ob_word(d, a.bits, item, it.w);
    const int x = it.x0 + l, g = it.row * d.nx + x;
    const bool in = x < d.nx, set = (word >> l) & 1ull;
    int ord = -1;
    if (set) {
        const int r = a.parent[g];
        if (r >= 0) ord = a.root_val[r];
    }
    if (in) a.labels[g] = ord;
    if (!word) return;   // (wave-uniform)
    // this cell's share of the fixed-point sums: the current result grid, voxels_objects_number[v][0..3]
    long long q[4] = {0, 0, 0, 0};
    if (ord >= 0 && ord < a.max_objects) {   // (a set cell of an object that has a record)
        const float4 r4 = s.res4[lv_of_true(d, g)];
        const float w = r4.x;
        if (w > 0.f && w < 4096.f) {   // (false for NaN)
            q[0] = ob_q20(w);
            const float u[3] = {r4.y, r4.z, r4.w};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p = __fmul_rn(w, u[k]);
                if (fabsf(u[k]) < INFINITY && fabsf(p) < 4096.f) q[1 + k] = ob_q20(p);   // (false for NaN)
            }
        }
    }
    // who adds: the first lane of every run whose object has a record -- or, where every such run of the word belongs to ONE object (the
    // rows of a large object), the first of them for all: its cells are then the ballot `mine`
    const u64 starts = word & ~(word << 1);
    const bool kept = ord >= 0 && ord < a.max_objects;
    const bool start = ((starts >> l) & 1ull) && kept;
    const u64 startm = __ballot(start);
    if (!startm) return;   // (wave-uniform)
    const int lead = (int)__ffsll((long long)startm) - 1;
    const int ord0 = __shfl(ord, lead, WAVE);
    const bool one = !__ballot(start && ord != ord0);   // (wave-uniform)
    const u64 all0 = __ballot(set && ord == ord0);
    const int len = start ? ob_run_len(word, l) : 1;
    const u64 mine = one ? all0 : (len >= 64 ? ~0ull : (1ull << len) - 1ull) << l;
    // inclusive prefix sums over the wave; a run's sum is the difference over its lanes, the word's sum the last lane's
    long long sum[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        long long v = q[k];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(v, o, WAVE);
            if (l >= o) v += t;
        }
        const long long hi = __shfl(v, one ? 63 : l + len - 1, WAVE), lo = __shfl_up(v, 1, WAVE);
        sum[k] = hi - (one || l == 0 ? 0 : lo);
    }
    if (!start || (one && l != lead)) return;
    const int cnt = (int)__popcll(mine), lo_x = it.x0 + (int)__ffsll((long long)mine) - 1, hi_x = it.x0 + 63 - (int)__clzll((long long)mine);
    dspmap_object* o = a.objects + ord;
    // the box: a plain look first -- the bounds only ever move outwards, so a value read late can only cost an atomic that changes nothing
    if (o->min_x > lo_x) atomicMin(&o->min_x, lo_x);
    if (o->max_x < hi_x) atomicMax(&o->max_x, hi_x);
    if (o->min_y > it.y) atomicMin(&o->min_y, it.y);
    if (o->max_y < it.y) atomicMax(&o->max_y, it.y);
    if (o->min_z > it.z) atomicMin(&o->min_z, it.z);
    if (o->max_z < it.z) atomicMax(&o->max_z, it.z);
    ob_add64(&o->sum_x, (long long)cnt * it.x0 + ob_lane_sum(mine));
    ob_add64(&o->sum_y, (long long)cnt * it.y);
    ob_add64(&o->sum_z, (long long)cnt * it.z);
    ob_add64(&o->mass_q, sum[0]);
#pragma unroll
    for (int k = 0; k < 3; ++k) ob_add64(&o->mom_q[k], sum[1 + k]);
}

// one thread per sample: the label-grid entry of the voxel that holds it (k_known_query's shape)
__global__ void __launch_bounds__(OB_TPB) k_objects_query(MapDims d, const int* __restrict__ labels, SampleOrigin org, int n,
                                                           const float4* __restrict__ q, int* __restrict__ out) {
    const unsigned i = blockIdx.x * OB_TPB + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 sm = q[i];
    int ord = -1;
    if (!(sm.x != sm.x || sm.y != sm.y || sm.z != sm.z)) {
        float px = sm.x, py = sm.y, pz = sm.z;
        origin_apply(org, px, py, pz);
        int g;
        if (voxel_of(d, px, py, pz, g)) ord = labels[g];
    }
    out[i] = ord;
}

void launch_objects(const LaunchCtx& c, const ObjectArgs& a) {
    const MapDims& d = c.d;
    const int n_items = (int)grid_layer_words(d);
    const int n_tiles = frontier_tiles(d.v_glob);
    const dim3 tpb(OB_TPB), words((unsigned)((n_items + OB_WAVES - 1) / OB_WAVES)), cells((unsigned)n_tiles);
    hipLaunchKernelGGL(k_objects_init, words, tpb, 0, c.stream, d, a, n_items);
    if (a.conn == 26) hipLaunchKernelGGL(k_objects_merge<true>, words, tpb, 0, c.stream, d, a, n_items);
    else hipLaunchKernelGGL(k_objects_merge<false>, words, tpb, 0, c.stream, d, a, n_items);
    hipLaunchKernelGGL(k_objects_flatten, cells, tpb, 0, c.stream, d, a);
    hipLaunchKernelGGL(k_objects_count, words, tpb, 0, c.stream, d, a, n_items);
    hipLaunchKernelGGL(k_objects_sums, cells, tpb, 0, c.stream, d, a);
    hipLaunchKernelGGL(k_objects_scan, dim3(1), tpb, 0, c.stream, a, n_tiles);
    hipLaunchKernelGGL(k_objects_emit, cells, tpb, 0, c.stream, d, a);
    hipLaunchKernelGGL(k_objects_accumulate, words, tpb, 0, c.stream, d, c.s, a, n_items);
}
void launch_objects_query(const LaunchCtx& c, const int* labels, const SampleOrigin& org, int n, const float4* q, int* out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_objects_query, dim3((unsigned)((n + OB_TPB - 1) / OB_TPB)), dim3(OB_TPB), 0, c.stream, c.d, labels, org, n, q, out);
}
