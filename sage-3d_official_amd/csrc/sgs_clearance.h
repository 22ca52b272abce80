// sgs_clearance.h — gfx950 kernels of the clearance map (sgs_clearance_map, sgs_clearance_query, include/sage_gs.h).
//
// The exact squared Euclidean distance transform of a batch of obstacle grids, in cells^2 as integers, and the position / path
// checks that look positions up in it: what the reference's collision_detector.py does on the host with SciPy's
// distance_transform_edt, a threshold at the robot radius and a pixel lookup per motion sub-step.
//
// Launches, all stream-ordered:
//   k_clear_counts   zeroes out_counts
//   k_clear_rows     blockIdx.y = map, blockIdx.x = a group of SGS_CLEAR_ROWS rows; a WAVE owns a row.  g[j][i] = the distance along
//                    x to the nearest obstacle of row j (SGS_CLEARANCE_NONE when the row has none), written to `work`; counts[0]
//                    (obstacle cells) is a popcount of the obstacle words
//   k_clear_cols     blockIdx.z = map, blockIdx.y = a group of SGS_CLEAR_ROWS rows, blockIdx.x = a word of 64 columns; a wave owns
//                    64 consecutive cells of a row.  d2[j][i] = min over rows j' with finite g of g[j'][i]^2 + (j - j')^2, written
//                    once; counts[1..3]
//   k_clear_query    a thread owns a segment
//
// Rows.  A wave walks its row in words of 64 cells: one ballot gives the obstacle word.  The words of the row are kept in LDS; a
// backward pass over them carries the position of the next obstacle to the right of every word, a forward pass the position of the
// last obstacle to the left; inside the word __clzll / __ffsll on the masked word give the nearest obstacle on either side.  The
// lanes beyond nx of the last word are neither cells nor obstacles.
// Columns.  A cell starts from its own g^2 (or NONE) and walks dy = 1, 2, ... up and down while dy^2 < best and a row exists in
// either direction; lanes are consecutive columns, so every row access is coalesced, and the wave loops while a ballot of
// "this lane still walks" is non-zero.  The walk is exact — a row at distance dy cannot give less than dy^2 — and short wherever an
// obstacle is near.  A map without any obstacle (counts[0] == 0 after k_clear_rows) is all NONE and is not walked.
// All arithmetic is on integers: a map's d2 depends on that map alone, not on the batch, the stride or how the kernels cut it.
// Counters: ballots and popcounts per wave, one LDS add per wave, one global add per workgroup.
//
// The intrinsics used are the ones every build has: ballot, __popcll, __ffsll, __clzll, 32-bit atomicAdd.
#pragma once
#include <math.h>
#include "sgs_common.h"

#define SGS_CLEAR_THREADS 256
#define SGS_CLEAR_ROWS (SGS_CLEAR_THREADS / 64)     // rows per workgroup: one per wave
#define SGS_CLEAR_MAX_NX 32768                      // cells of a row (and rows of a map): g^2 + dy^2 <= 2 * 32767^2 fits 32 bits
#define SGS_CLEAR_MAX_WORDS (SGS_CLEAR_MAX_NX / 64) // obstacle words of a row
#define SGS_CLEAR_MAX_MAPS 65535                    // maps per launch (gridDim.y / gridDim.z); more are issued in chunks
#define SGS_CLEAR_NONE 0xFFFFFFFFu
#define SGS_CLEAR_SRC_MASK8 0
#define SGS_CLEAR_SRC_TOPDOWN 1
#define SGS_CLEAR_UNSEEN_BLOCKS 1u
#define SGS_CLEAR_NEGATE 1u
#define SGS_CLEAR_FLIP_X 2u
#define SGS_CLEAR_FLIP_Y 4u

namespace sgs {

struct ClearanceJob {
    const void* src;                       // n_maps maps, stride elements apart: uint8 [ny][nx] or uint32 [ny][nx][2]
    unsigned* work;                        // [n_maps][ny][nx]: g
    unsigned* d2;                          // [n_maps][ny][nx]
    unsigned* counts;                      // [n_maps][4]
    long long stride;
    long long map0;                        // the first map of this launch
    int nx, ny, n_maps, kind;
    unsigned min_hits, unseen_blocks, max_d2;
};

// Whether cell (i, j) of map m is an obstacle.
__device__ __forceinline__ bool clearance_obstacle(const ClearanceJob& J, long long m, int j, int i) {
    const long long cell = (long long)j * J.nx + i;
    if (J.kind == SGS_CLEAR_SRC_MASK8) return static_cast<const unsigned char*>(J.src)[m * J.stride + cell] != 0;
    const unsigned* c = static_cast<const unsigned*>(J.src) + m * J.stride + 2 * cell;
    const unsigned free_hits = c[0], occ = c[1];
    return occ >= J.min_hits || (J.unseen_blocks && free_hits < J.min_hits);
}

__global__ __launch_bounds__(SGS_CLEAR_THREADS) void k_clear_counts(unsigned* counts, long long words) {
    const long long step = (long long)gridDim.x * SGS_CLEAR_THREADS;
    for (long long i = (long long)blockIdx.x * SGS_CLEAR_THREADS + threadIdx.x; i < words; i += step) counts[i] = 0;
}

__global__ __launch_bounds__(SGS_CLEAR_THREADS) void k_clear_rows(ClearanceJob J) {
    __shared__ unsigned long long s_word[SGS_CLEAR_ROWS][SGS_CLEAR_MAX_WORDS];
    __shared__ int s_next[SGS_CLEAR_ROWS][SGS_CLEAR_MAX_WORDS];
    __shared__ unsigned s_obstacles;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m = J.map0 + blockIdx.y;
    const int j = (int)blockIdx.x * SGS_CLEAR_ROWS + wave;
    const bool row = j < J.ny;                                                     // (wave-uniform)
    const int words = (J.nx + 63) >> 6;
    if (tid == 0) s_obstacles = 0;
    __syncthreads();

    // 1. the obstacle words of the row: the lanes beyond nx are no cells
    unsigned n_obstacles = 0;
    for (int w = 0; w < words; ++w) {
        const int i = (w << 6) + lane;
        const bool ob = row && i < J.nx && clearance_obstacle(J, m, j, i);
        const unsigned long long word = __ballot(ob);
        n_obstacles += (unsigned)__popcll(word);
        if (lane == 0) s_word[wave][w] = word;
    }
    if (lane == 0 && n_obstacles) atomicAdd(&s_obstacles, n_obstacles);
    __syncthreads();

    // 2. right to left: the position of the first obstacle in the words after w (-1: none), shared out over the lanes by words
    if (lane == 0) {
        int next = -1;
        for (int w = words - 1; w >= 0; --w) {
            s_next[wave][w] = next;
            const unsigned long long word = s_word[wave][w];
            if (word) next = (w << 6) + __ffsll((long long)word) - 1;
        }
    }
    __syncthreads();

    // 3. left to right: the last obstacle before the word is carried; inside the word the masked word decides
    unsigned* g = J.work + (m * J.ny + j) * (long long)J.nx;
    int last = -1;
    for (int w = 0; w < words; ++w) {
        const int i = (w << 6) + lane;
        const unsigned long long word = s_word[wave][w];
        const unsigned long long at_or_left = word & (~0ull >> (63 - lane));
        const unsigned long long at_or_right = word & (~0ull << lane);
        unsigned left = SGS_CLEAR_NONE, right = SGS_CLEAR_NONE;
        if (at_or_left) left = (unsigned)(lane - (63 - __clzll((long long)at_or_left)));
        else if (last >= 0) left = (unsigned)(i - last);
        const int next = s_next[wave][w];
        if (at_or_right) right = (unsigned)(__ffsll((long long)at_or_right) - 1 - lane);
        else if (next >= 0) right = (unsigned)(next - i);
        if (row && i < J.nx) g[i] = left < right ? left : right;
        if (word) last = (w << 6) + 63 - __clzll((long long)word);
    }
    if (tid == 0 && s_obstacles) atomicAdd(&J.counts[4 * m], s_obstacles);
}

__global__ __launch_bounds__(SGS_CLEAR_THREADS) void k_clear_cols(ClearanceJob J) {
    __shared__ unsigned s_cnt[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m = J.map0 + blockIdx.z;
    const int j = (int)blockIdx.y * SGS_CLEAR_ROWS + wave;
    const int i = ((int)blockIdx.x << 6) + lane;
    const bool valid = j < J.ny && i < J.nx;
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    const long long cells = (long long)J.nx * J.ny;
    const unsigned* g = J.work + m * cells + (valid ? i : 0);                       // column i of the map's g
    unsigned best = SGS_CLEAR_NONE;
    if (J.counts[4 * m] != 0) {                                                    // (block-uniform: k_clear_rows has finished)
        if (valid) {
            const unsigned own = g[(long long)j * J.nx];
            if (own != SGS_CLEAR_NONE) best = own * own;
        }
        const unsigned up_rows = valid ? (unsigned)j : 0u, down_rows = valid ? (unsigned)(J.ny - 1 - j) : 0u;
        for (unsigned dy = 1;; ++dy) {
            const unsigned dy2 = dy * dy;                                          // dy <= 32767
            const bool walks = dy2 < best && (dy <= up_rows || dy <= down_rows);
            if (!__ballot(walks)) break;
            if (walks) {
                if (dy <= up_rows) {
                    const unsigned v = g[(long long)(j - (int)dy) * J.nx];
                    if (v != SGS_CLEAR_NONE) { const unsigned c = v * v + dy2; best = c < best ? c : best; }
                }
                if (dy <= down_rows) {
                    const unsigned v = g[(long long)(j + (int)dy) * J.nx];
                    if (v != SGS_CLEAR_NONE) { const unsigned c = v * v + dy2; best = c < best ? c : best; }
                }
            }
        }
    }
    if (valid) J.d2[m * cells + (long long)j * J.nx + i] = best;

    const unsigned n_near = (unsigned)__popcll(__ballot(valid && best > 0u && best <= J.max_d2));
    const unsigned n_far = (unsigned)__popcll(__ballot(valid && best > J.max_d2 && best < SGS_CLEAR_NONE));
    const unsigned n_none = (unsigned)__popcll(__ballot(valid && best == SGS_CLEAR_NONE));
    if (lane == 0) {
        if (n_near) atomicAdd(&s_cnt[1], n_near);
        if (n_far) atomicAdd(&s_cnt[2], n_far);
        if (n_none) atomicAdd(&s_cnt[3], n_none);
    }
    __syncthreads();
    if (tid >= 1 && tid < 4 && s_cnt[tid]) atomicAdd(&J.counts[4 * m + tid], s_cnt[tid]);
}

// ---- sgs_clearance_query ------------------------------------------------------------------------------------------------------------
struct ClearanceQuery {
    const unsigned* d2;                    // one map [ny][nx]
    const double* segs;                    // [n][4]: x0, y0, x1, y1
    unsigned* out;                         // [n][2]: first colliding sample (from 1) or 0; d2 under the end point or NONE
    long long n;
    int nx, ny, margin, n_samples;
    double min_x, min_y, sum_x, sum_y, scale;
    unsigned flags, max_d2;
};

// One coordinate of a sample to its pixel: rint of a true division; false when the pixel is outside beyond the margin (NaN and
// +-inf are).  Inside the margin it is clamped to the border.
__device__ __forceinline__ bool clearance_pixel(double v, double lo, double scale, int n, int margin, int* p) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double q = rint((v - lo) / scale);
    if (!(q >= -(double)margin && q < (double)n + (double)margin)) return false;
    *p = q < 0.0 ? 0 : q > (double)(n - 1) ? n - 1 : (int)q;
    return true;
}

// The d2 under the point (x, y) of the caller's frame, NONE when it is outside beyond the margin; *hit: the point collides.
__device__ __forceinline__ unsigned clearance_sample(const ClearanceQuery& Q, double x, double y, bool* hit) {
    if (Q.flags & SGS_CLEAR_NEGATE) { x = -x; y = -y; }
    if (Q.flags & SGS_CLEAR_FLIP_X) x = Q.sum_x - x;
    if (Q.flags & SGS_CLEAR_FLIP_Y) y = Q.sum_y - y;
    int px = 0, py = 0;
    const bool in_x = clearance_pixel(x, Q.min_x, Q.scale, Q.nx, Q.margin, &px);
    const bool in_y = clearance_pixel(y, Q.min_y, Q.scale, Q.ny, Q.margin, &py);
    if (!(in_x && in_y)) { *hit = true; return SGS_CLEAR_NONE; }
    const unsigned v = Q.d2[(long long)py * Q.nx + px];
    *hit = v <= Q.max_d2;
    return v;
}

__global__ __launch_bounds__(SGS_CLEAR_THREADS) void k_clear_query(ClearanceQuery Q) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const long long k = (long long)blockIdx.x * SGS_CLEAR_THREADS + threadIdx.x;
    if (k >= Q.n) return;
    const double x0 = Q.segs[4 * k], y0 = Q.segs[4 * k + 1], x1 = Q.segs[4 * k + 2], y1 = Q.segs[4 * k + 3];
    unsigned first = 0, under_end = SGS_CLEAR_NONE;
    bool hit = false, found = false;
    if (Q.n_samples <= 1) {                                                        // the end point itself, untouched
        under_end = clearance_sample(Q, x1, y1, &hit);
        first = hit ? 1u : 0u;
    } else {
        const double n = (double)Q.n_samples;
        for (int s = 1; s <= Q.n_samples; ++s) {
            if (found && s < Q.n_samples) s = Q.n_samples;                         // after the first hit only the end point is still wanted
            const double t = (double)s / n;
            const double x = x0 * (1.0 - t) + x1 * t, y = y0 * (1.0 - t) + y1 * t;
            const unsigned v = clearance_sample(Q, x, y, &hit);
            if (hit && !found) { found = true; first = (unsigned)s; }
            if (s == Q.n_samples) under_end = v;
        }
    }
    Q.out[2 * k] = first;
    Q.out[2 * k + 1] = under_end;
}

}  // namespace sgs
