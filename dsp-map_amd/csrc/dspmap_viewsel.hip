// dspmap_viewsel.hip -- the joint gain of views (dspmap_score_view_sets*, dspmap_select_views*; semantics next to them in include/dspmap.h):
// what a SET of views sees together, and the greedy choice of the k views that see the most unknown space together.  The reference has
// no counterpart.  Every view's seen set S_i is a bit mask [nz][ny][W] in the cast grid's word layout, written by the MASK instantiation
// of k_view_score (dspmap_view.hip) behind a memset; everything here is OR, AND and popcount over such words.
//
//   k_vs_unknown   UNK: a wave per word of a row, the ballot of "age is -1 or > max_age" (k_known_mask's predicate); bits past nx are 0.
//   k_vs_sets      one workgroup per (set, chunk of words): a thread ORs its word over the members, counts the union and the union under
//                  UNK (the union of the U_i = S_i & UNK is the union of the S_i under UNK: every view reads the same ages); chunk 0 counts
//                  the members whose status is OK.  k_view_score's tail: wave sum, LDS, then one integer atomic per workgroup and
//                  non-zero counter into the zeroed score.  With `avail`, the selection's start: avail = UNK & ~union of the fixed views.
//   the greedy rounds, three launches each, no host in between and no kernel that waits for another:
//   k_vs_gain      one workgroup per (candidate, chunk): popcount(S_i & avail) into gain[i].  avail = UNK & ~C, so this is |U_i \ C|
//                  without forming U_i: the masks are written once and only read afterwards.
//   k_vs_pick      ONE workgroup: the maximum of the key (gain << 32) | (0xffffffff - i) -- the largest gain, the smallest index among
//                  equals --, the pick record, and gain cleared for the next round.  covered = the previous record's + the gain.
//   k_vs_cover     avail &= ~S_pick, the pick read from the record; nothing after an empty pick.  avail then stays as it is, so every
//                  later round finds the same gains below min_gain and is empty too: no flag says "stopped".
// All counts are integers of exactly defined predicates: no result depends on the chunking.  Nothing of the map, the grid or the layer is
// written.
#include "dspmap_device.h"
#include "dspmap_grid.h"
#include "dspmap_internal.h"
#include "dspmap_known_slots.h"   // kn_cell, kn_age

#define VS_TPB 256
#define VS_WAVES (VS_TPB / 64)

__global__ void __launch_bounds__(VS_TPB) k_vs_unknown(MapDims d, KnownArgs a, int max_age, u64* __restrict__ unk, int n_items) {
    const int item = (int)blockIdx.x * VS_WAVES + ((int)threadIdx.x >> 6);
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
    if (l == 0) unk[item] = word;
}

// out [n_sets] zeroed by the caller; scores [n_sets * set_size] as k_view_score left them; avail: NULL, or (n_sets == 1) [lw]
__global__ void __launch_bounds__(VS_TPB) k_vs_sets(int lw, int n_sets, int set_size, int chunks, const u64* __restrict__ masks,
                                                     const u64* __restrict__ unk, const int4* __restrict__ scores, int4* __restrict__ out,
                                                     u64* __restrict__ avail) {
    __shared__ int s_cnt[3];
    const int set = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    if (set >= n_sets) return;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const u64* m0 = masks + (size_t)set * set_size * (size_t)lw;
    int seen_n = 0, unk_n = 0, ok_n = 0;
    for (int w = chunk * VS_TPB + (int)threadIdx.x; w < lw; w += chunks * VS_TPB) {
        u64 u = 0;
        for (int j = 0; j < set_size; ++j) u |= m0[(size_t)j * lw + w];
        const u64 k = unk[w];
        seen_n += (int)__popcll(u);
        unk_n += (int)__popcll(u & k);
        if (avail) avail[w] = k & ~u;
    }
    if (chunk == 0)
        for (int j = threadIdx.x; j < set_size; j += VS_TPB) ok_n += scores[(size_t)set * set_size + j].w == DSPMAP_VIEW_OK ? 1 : 0;
    seen_n = wave_sum_i(seen_n); unk_n = wave_sum_i(unk_n); ok_n = wave_sum_i(ok_n);
    if (lane_id() == 0) {
        if (seen_n) atomicAdd(&s_cnt[0], seen_n);
        if (unk_n) atomicAdd(&s_cnt[1], unk_n);
        if (ok_n) atomicAdd(&s_cnt[2], ok_n);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&((int*)(out + set))[threadIdx.x], s_cnt[threadIdx.x]);
}

// gain [n_cand] zero on entry (the caller's memset, then k_vs_pick); masks: those of the candidates
__global__ void __launch_bounds__(VS_TPB) k_vs_gain(int lw, int n_cand, int chunks, const u64* __restrict__ masks, const u64* __restrict__ avail,
                                                     int* __restrict__ gain) {
    __shared__ int s_cnt;
    const int c = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    if (c >= n_cand) return;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const u64* mk = masks + (size_t)c * lw;
    int g = 0;
    for (int w = chunk * VS_TPB + (int)threadIdx.x; w < lw; w += chunks * VS_TPB) g += (int)__popcll(mk[w] & avail[w]);
    g = wave_sum_i(g);
    if (lane_id() == 0 && g) atomicAdd(&s_cnt, g);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&gain[c], s_cnt);
}

// round r: picks[r] from gain [n_cand] (candidate c is view n_fixed + c); fixed: the score of the fixed views' set, .y = |C_0|
__global__ void __launch_bounds__(VS_TPB) k_vs_pick(int n_fixed, int n_cand, int r, int min_gain, int* __restrict__ gain,
                                                     const int4* __restrict__ fixed, int4* __restrict__ picks) {
    __shared__ u64 s_key;
    if (threadIdx.x == 0) s_key = 0;
    __syncthreads();
    u64 best = 0;
    for (int c = threadIdx.x; c < n_cand; c += VS_TPB) {
        const u64 key = ((u64)(unsigned)gain[c] << 32) | (u64)(0xffffffffu - (unsigned)(n_fixed + c));
        best = key > best ? key : best;
        gain[c] = 0;
    }
    if (best) atomicMax(&s_key, best);
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 key = s_key;
        const int g = (int)(key >> 32);
        const int covered = r == 0 ? fixed->y : picks[r - 1].z;
        picks[r] = g >= min_gain ? make_int4((int)(0xffffffffu - (unsigned)key), g, covered + g, 0) : make_int4(-1, 0, covered, 0);
    }
}

// masks: those of ALL views (the record holds a view index)
__global__ void __launch_bounds__(VS_TPB) k_vs_cover(int lw, const u64* __restrict__ masks, const int4* __restrict__ pick, u64* __restrict__ avail) {
    const int v = pick->x;   // (uniform over the grid)
    if (v < 0) return;
    const int w = (int)(blockIdx.x * VS_TPB + threadIdx.x);   // one thread per word (lw < 2^31: the grid has room)
    if (w < lw) avail[w] &= ~masks[(size_t)v * lw + w];
}

// workgroups per item (a set, a candidate) of a batch of n: as view_chunks -- about four workgroups per CU in all, no more than the
// layer has words for (a chunk of fewer than VS_TPB words idles threads).  forced > 0 (DSPMAP_P_VIEW_CHUNKS): that many, at most 64 as
// the parameter says, whatever the layer's size -- a chunk that starts past the last word does nothing
int viewsel_chunks(int lw, int n, int n_cu, int forced) {
    long long most = ((long long)lw + VS_TPB - 1) / VS_TPB;
    if (most < 1) most = 1;
    if (forced > 0) most = 64;
    long long c = forced > 0 ? forced : ((long long)(n_cu > 0 ? n_cu : 256) * 4 + n - 1) / (n > 0 ? n : 1);
    if (c > most) c = most;
    if (c < 1) c = 1;
    while (c > 1 && (long long)n * c > 0x7fffffffll) --c;
    return (int)c;
}

void launch_viewsel_unknown(const MapDims& d, hipStream_t stream, const KnownArgs& a, int max_age, u64* unk) {
    const int n_items = (int)grid_layer_words(d);
    hipLaunchKernelGGL(k_vs_unknown, dim3((unsigned)((n_items + VS_WAVES - 1) / VS_WAVES)), dim3(VS_TPB), 0, stream, d, a, max_age, unk, n_items);
}
void launch_viewsel_sets(hipStream_t stream, int lw, int n_sets, int set_size, int chunks, const u64* masks, const u64* unk,
                         const dspmap_view_score* scores, dspmap_view_set_score* out, u64* avail) {
    if (n_sets <= 0) return;
    hipLaunchKernelGGL(k_vs_sets, dim3((unsigned)((long long)n_sets * chunks)), dim3(VS_TPB), 0, stream, lw, n_sets, set_size, chunks, masks, unk,
                       (const int4*)scores, (int4*)out, avail);
}
void launch_viewsel_round(hipStream_t stream, int lw, int n_fixed, int n_cand, int chunks, int r, int min_gain, const u64* masks, u64* avail,
                          int* gain, const dspmap_view_set_score* fixed, dspmap_view_pick* picks) {
    if (n_cand > 0)
        hipLaunchKernelGGL(k_vs_gain, dim3((unsigned)((long long)n_cand * chunks)), dim3(VS_TPB), 0, stream, lw, n_cand, chunks,
                           masks + (size_t)n_fixed * lw, avail, gain);
    hipLaunchKernelGGL(k_vs_pick, dim3(1), dim3(VS_TPB), 0, stream, n_fixed, n_cand, r, min_gain, gain, (const int4*)fixed, (int4*)picks);
    if (n_cand > 0)
        hipLaunchKernelGGL(k_vs_cover, dim3((unsigned)(((long long)lw + VS_TPB - 1) / VS_TPB)), dim3(VS_TPB), 0, stream, lw, masks, (const int4*)(picks + r), avail);
}
