// sgs_topdown.h — gfx950 kernels of the top-down seen map (sgs_topdown_map, sgs_topdown_summary, include/sage_gs.h).
//
// Depth frames (fp32 per pixel, as sgs_render_mesh_depth* writes them) are unprojected through twelve numbers per frame and binned
// by height into a grid of cells: per cell a count of "free" hits (the floor band) and of "occupied" hits (the obstacle band).  THIS
// PROJECT'S OWN definition, like the id channel, the object table and the similarity row: the reference counts the cells the agent
// stood in (measures.py:399-437) and has no map of what it saw.
//
// Launches, all stream-ordered:
//   k_topdown_clear     zeroes the per-frame counters, and the grid when SGS_TOPDOWN_CLEAR is set
//   k_topdown_map       blockIdx.y = frame, blockIdx.x = a region of SGS_TOPDOWN_REGION consecutive pixels of that frame (row-major); a
//                       region never spans two frames
//   k_topdown_sum_clear / k_topdown_sum   the four numbers of sgs_topdown_summary
//
// Per pixel the arithmetic is fp32, every multiply and add rounded once in the order the header writes it (contraction is off), and
// there is no division: the same bits on every build.  What is accumulated is an integer count, so every contribution commutes: a grid
// depends on the frames, the matrices and the parameters alone, not on how a frame is cut into regions, waves and runs.  The reduction
// has the three levels of k_obj_reduce (sgs_objects.h), keyed by key = 2 (j nx + i) + channel (0 free, 1 occupied):
//   lanes      a wave holds 64 consecutive pixels.  A camera that looks along a floor or at a wall puts neighbouring pixels into one
//              cell: lanes next to each other with one key form a RUN, found with a ballot of "not binned / key differs from the
//              previous lane"; the run's head lane contributes the run's length.  A run carries nothing but its key and its length,
//              so — unlike k_obj_reduce's, which carry x and y — it may continue from the end of one image row into the next.
//   LDS        a table of SGS_TOPDOWN_SLOTS slots per workgroup, slot = topdown_slot(key).  Ownership needs no compare-and-swap: every
//              run head of the region first proposes atomicMax(&s_key[slot], key + 1); after a barrier the key is final, and the runs
//              whose key owns its slot add their length there.  Runs whose key lost its slot (more keys in the region than slots, or
//              keys that collide) add straight to the global grid — the same count, so the result is the same.
//   global     after a barrier, one atomicAdd per (workgroup, key that owned a slot), and one per counter.
// The pixels are classified with ballots: the four per-frame counters cost one popcount per wave and class, one LDS add per wave and
// one global add per workgroup.
//
// The atomics used are the ones every build has: atomicAdd (32- and 64-bit) and unsigned atomicMax.
#pragma once
#include "sgs_common.h"

#define SGS_TOPDOWN_THREADS 256
#define SGS_TOPDOWN_PER_THREAD 16
#define SGS_TOPDOWN_REGION (SGS_TOPDOWN_THREADS * SGS_TOPDOWN_PER_THREAD)   // pixels of a frame per workgroup
#define SGS_TOPDOWN_SLOT_BITS 10
#define SGS_TOPDOWN_SLOTS (1 << SGS_TOPDOWN_SLOT_BITS)                      // entries of the workgroup's LDS table (8 bytes each)
#define SGS_TOPDOWN_HASH 0x9E3779B1u                                        // slot = (key * SGS_TOPDOWN_HASH) >> (32 - SGS_TOPDOWN_SLOT_BITS)
#define SGS_TOPDOWN_NO_KEY 0xFFFFFFFFu                                      // a pixel that is not binned (keys are below 2^31 - 1)
#define SGS_TOPDOWN_MAX_FRAMES 65535                                        // frames per k_topdown_map launch (gridDim.y); more are issued in chunks
#define SGS_TOPDOWN_SUM_BLOCKS 1024                                         // most workgroups of k_topdown_sum (it strides)

namespace sgs {

struct TopdownJob {
    const float* depth;                    // n_frames frames, stride elements apart
    const float* P;                        // [n_frames][12]: rows (a_k, b_k, c_k), k = 0, 1, 2, then t_0, t_1, t_2
    unsigned* grid;                        // [ny][nx][2]: free hits, occupied hits
    unsigned* counts;                      // [n_frames][4]: z out of range, outside the grid, in no band, binned
    long long stride;
    int W, H, n_frames, nx, ny;
    float origin_x, origin_y, inv;         // inv = 1.0f / cell_size, computed once on the host
    float min_z, max_z, free_lo, free_hi, occ_lo, occ_hi;
    unsigned clear;
};

__device__ __forceinline__ unsigned topdown_slot(unsigned key) { return (key * SGS_TOPDOWN_HASH) >> (32 - SGS_TOPDOWN_SLOT_BITS); }

// The class of one pixel (0 z out of range, 1 outside the grid, 2 in no height band, 3 binned) and, for class 3, its key.
__device__ __forceinline__ int topdown_classify(const TopdownJob& J, const float* P, unsigned x, unsigned y, float z, unsigned* key) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    *key = SGS_TOPDOWN_NO_KEY;
    if (!(J.min_z <= z && z <= J.max_z)) return 0;
    const float fx = (float)x, fy = (float)y;
    const float d0 = (fx * P[0] + fy * P[1]) + P[2];
    const float d1 = (fx * P[3] + fy * P[4]) + P[5];
    const float d2 = (fx * P[6] + fy * P[7]) + P[8];
    const float p0 = z * d0 + P[9];
    const float p1 = z * d1 + P[10];
    const float h = z * d2 + P[11];
    const float u = (p0 - J.origin_x) * J.inv;
    const float v = (p1 - J.origin_y) * J.inv;
    const bool inside = u >= 0.0f && u < (float)J.nx && v >= 0.0f && v < (float)J.ny;
    if (!inside) return 1;
    const int i = (int)u, j = (int)v;
    const bool is_free = J.free_lo <= h && h <= J.free_hi;
    const bool is_occ = !is_free && J.occ_lo < h && h <= J.occ_hi;
    if (!is_free && !is_occ) return 2;
    *key = 2u * ((unsigned)j * (unsigned)J.nx + (unsigned)i) + (is_occ ? 1u : 0u);
    return 3;
}

// The counters become 0; with SGS_TOPDOWN_CLEAR so does the grid.
__global__ __launch_bounds__(SGS_TOPDOWN_THREADS) void k_topdown_clear(TopdownJob J) {
    const long long step = (long long)gridDim.x * SGS_TOPDOWN_THREADS;
    const long long first = (long long)blockIdx.x * SGS_TOPDOWN_THREADS + threadIdx.x;
    for (long long i = first; i < 4ll * J.n_frames; i += step) J.counts[i] = 0;
    if (J.clear) {
        const long long words = 2ll * J.nx * J.ny;
        for (long long i = first; i < words; i += step) J.grid[i] = 0;
    }
}

__global__ __launch_bounds__(SGS_TOPDOWN_THREADS) void k_topdown_map(TopdownJob J) {
    __shared__ unsigned s_key[SGS_TOPDOWN_SLOTS], s_n[SGS_TOPDOWN_SLOTS], s_cnt[4];
    __shared__ float s_P[12];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long f = blockIdx.y;
    const unsigned W = (unsigned)J.W, HW = (unsigned)J.W * (unsigned)J.H;          // H W <= 2^31 - 1
    const float* depth = J.depth + f * J.stride;

    for (int s = tid; s < SGS_TOPDOWN_SLOTS; s += SGS_TOPDOWN_THREADS) { s_key[s] = 0; s_n[s] = 0; }
    if (tid < 4) s_cnt[tid] = 0;
    if (tid < 12) s_P[tid] = J.P[12 * f + tid];
    __syncthreads();

    // pixel k of this thread is p0 + k * SGS_TOPDOWN_THREADS (below 2^31 + SGS_TOPDOWN_REGION: fits 32 bits): the lanes of a wave hold
    // 64 consecutive pixels at every k
    const unsigned p0 = blockIdx.x * (unsigned)SGS_TOPDOWN_REGION + (unsigned)tid;
    float z[SGS_TOPDOWN_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SGS_TOPDOWN_PER_THREAD; ++k) {
        const unsigned p = p0 + (unsigned)k * SGS_TOPDOWN_THREADS;
        z[k] = p < HW ? depth[p] : 0.0f;
    }

    // 1. classify; every key of the region proposes itself for its slot (one lane per change of key covers every key a wave holds)
    const unsigned step_y = SGS_TOPDOWN_THREADS / W, step_x = SGS_TOPDOWN_THREADS % W;
    unsigned y = p0 / W, x = p0 - y * W;
    unsigned key[SGS_TOPDOWN_PER_THREAD];
    unsigned n_cls[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < SGS_TOPDOWN_PER_THREAD; ++k) {
        const bool valid = p0 + (unsigned)k * SGS_TOPDOWN_THREADS < HW;
        const int cls = valid ? topdown_classify(J, s_P, x, y, z[k], &key[k]) : -1;
        if (!valid) key[k] = SGS_TOPDOWN_NO_KEY;
#pragma unroll
        for (int c = 0; c < 4; ++c) n_cls[c] += (unsigned)__popcll(__ballot(cls == c));
        const unsigned prev = __shfl_up(key[k], 1);
        if (key[k] != SGS_TOPDOWN_NO_KEY && (lane == 0 || key[k] != prev)) atomicMax(&s_key[topdown_slot(key[k])], key[k] + 1u);
        x += step_x; y += step_y;
        if (x >= W) { x -= W; y += 1u; }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (n_cls[c]) atomicAdd(&s_cnt[c], n_cls[c]);
    }
    __syncthreads();

    // 2. runs
#pragma unroll
    for (int k = 0; k < SGS_TOPDOWN_PER_THREAD; ++k) {
        const unsigned v = key[k];
        const bool binned = v != SGS_TOPDOWN_NO_KEY;
        const unsigned prev = __shfl_up(v, 1);
        const bool head = binned && (lane == 0 || v != prev);
        const unsigned long long starts = __ballot(!binned || head);               // where a segment begins (bit 0 is always set)
        const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
        const int next = above ? lane + __ffsll((long long)above) : 64;            // the lane that begins the next segment
        if (head) {
            const unsigned len = (unsigned)(next - lane);
            const unsigned s = topdown_slot(v);
            if (s_key[s] == v + 1u) atomicAdd(&s_n[s], len);
            else atomicAdd(&J.grid[v], len);
        }
    }
    __syncthreads();

    // 3. one global add per key that owned a slot, and one per counter
    for (int s = tid; s < SGS_TOPDOWN_SLOTS; s += SGS_TOPDOWN_THREADS)
        if (s_n[s]) atomicAdd(&J.grid[s_key[s] - 1u], s_n[s]);
    if (tid < 4 && s_cnt[tid]) atomicAdd(&J.counts[4 * f + tid], s_cnt[tid]);
}

// ---- sgs_topdown_summary: out[0] cells with occupied >= min_hits, out[1] cells with occupied < min_hits <= free, out[2] free hits,
// out[3] occupied hits.  The two cell counts are a ballot and a popcount per wave; the two sums are folded across the wave with
// shuffles; one set of four 64-bit adds per workgroup.
__global__ void k_topdown_sum_clear(unsigned long long* out) {
    if (threadIdx.x < 4) out[threadIdx.x] = 0;
}

__global__ __launch_bounds__(SGS_TOPDOWN_THREADS) void k_topdown_sum(const unsigned* grid, long long cells, unsigned min_hits, unsigned long long* out) {
    __shared__ unsigned long long s_part[SGS_TOPDOWN_THREADS / 64][4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long step = (long long)gridDim.x * SGS_TOPDOWN_THREADS;
    unsigned long long n_occ = 0, n_free = 0, sum_free = 0, sum_occ = 0;
    // every lane of a wave makes the same number of trips (the ballots need them all): the bound is the wave's first cell
    for (long long base = (long long)blockIdx.x * SGS_TOPDOWN_THREADS + (tid - lane); base < cells; base += step) {
        const long long c = base + lane;
        const bool valid = c < cells;
        const unsigned fr = valid ? grid[2 * c] : 0u, oc = valid ? grid[2 * c + 1] : 0u;
        n_occ += (unsigned long long)__popcll(__ballot(valid && oc >= min_hits));
        n_free += (unsigned long long)__popcll(__ballot(valid && oc < min_hits && fr >= min_hits));
        sum_free += fr; sum_occ += oc;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum_free += __shfl_xor(sum_free, d);
        sum_occ += __shfl_xor(sum_occ, d);
    }
    if (lane == 0) { s_part[wave][0] = n_occ; s_part[wave][1] = n_free; s_part[wave][2] = sum_free; s_part[wave][3] = sum_occ; }
    __syncthreads();
    if (tid < 4) {
        unsigned long long t = 0;
        for (int w = 0; w < SGS_TOPDOWN_THREADS / 64; ++w) t += s_part[w][tid];
        if (t) atomicAdd(&out[tid], t);
    }
}

}  // namespace sgs
