// sgs_similarity.h — gfx950 kernels of the image similarity (sgs_image_similarity, include/sage_gs.h).
//
// Windowed SSIM and squared error of fp32 frames against uint8 target pictures, one 64-byte row per frame.  THIS PROJECT'S OWN
// definition, like the id channel and the object table: the reference names the measure (task_types.py:183-208) and returns a
// placeholder.  The definition — levels, the 11 x 11 integer window, the five moments, the four int64 terms, one fp64 quotient per
// window, floor to 30 fractional bits — is in include/sage_gs.h; nothing here may depart from it by a bit.
//
// Two stream-ordered launches:
//   k_sim_clear    writes every frame's row: n_windows, n_pixels, zeros (what the output held does not matter)
//   k_sim_reduce   blockIdx.y = frame, blockIdx.x = a tile of SGS_SIM_TILE_W x SGS_SIM_TILE_H windows (row-major over the frame's tiles)
//
// A workgroup of k_sim_reduce:
//   load       the (TILE_W + 10) x (TILE_H + 10) pixels under its windows, ONCE, both pictures, all three channels, into LDS as
//              16-bit pairs (x | y << 8): the frame's floats through sim_level, the target's bytes as they are; pixels beyond the
//              frame are 0 and belong to no window that counts.  The same walk takes (x - y)^2 of the pixels the tile OWNS —
//              those under its window origins, and in the last tile column / row also the ten beyond — so every pixel of the
//              frame is counted once.
//   per channel
//     horizontal  the five moments of every row of the tile along x, 32 bits (2048 * 255^2 < 2^28), into LDS
//     vertical    a thread takes one column and SGS_SIM_ROWS consecutive window rows: 10 + SGS_SIM_ROWS reads per moment, the first
//                 moments in 32 bits (2^22 * 255 < 2^30), the second in 64 (v_mad_u64_u32); then q per window in fp64
//     reduce      q over the wave by shuffles, one 64-bit LDS add per wave
//   send       six 64-bit global atomics per workgroup: ssim_q[3], sse[3]
// Every pixel is read from memory about once (the 10-pixel aprons of neighbouring tiles overlap: 1.7 reads per pixel, most of them
// cache hits), not 121 times.  All sums are integers, so a row does not depend on the order in which tiles and waves arrive.
//
// The fp64 expression holds no sum next to a product, so there is nothing a compiler could contract: hipcc and the host compiler of
// the CPU test build produce the same q from the same levels.  The level is k_pack_rgba8's expression, fused or not as it is there.
#pragma once
#include <cmath>

#include "sgs_common.h"

#define SGS_SIM_THREADS 256
#define SGS_SIM_TAPS SGS_SIM_WINDOW                                // 11
#define SGS_SIM_IN_W (SGS_SIM_TILE_W + SGS_SIM_TAPS - 1)           // pixels of a tile across
#define SGS_SIM_IN_H (SGS_SIM_TILE_H + SGS_SIM_TAPS - 1)           // ... and down
#define SGS_SIM_ROWS (SGS_SIM_TILE_W * SGS_SIM_TILE_H / SGS_SIM_THREADS)      // window rows of one column per thread
#define SGS_SIM_T_BITS 22                                          // total weight of a window T = 2^22
#define SGS_SIM_C1 114393189753815ll                               // (0.01 * 255)^2 T^2, rounded
#define SGS_SIM_C2 1029538707784335ll                              // (0.03 * 255)^2 T^2, rounded
#define SGS_SIM_MAX_FRAMES 65535                                   // frames per k_sim_reduce launch (gridDim.y); more are issued in chunks

namespace sgs {

static_assert(SGS_SIM_TAPS == 11, "the taps below are eleven");
static_assert((SGS_SIM_TILE_W & (SGS_SIM_TILE_W - 1)) == 0 && SGS_SIM_THREADS % SGS_SIM_TILE_W == 0, "a wave holds whole rows of columns");
static_assert(SGS_SIM_ROWS * SGS_SIM_THREADS == SGS_SIM_TILE_W * SGS_SIM_TILE_H, "every window of a tile has one thread");
static_assert((SGS_SIM_IN_W * SGS_SIM_IN_H * 3 + SGS_SIM_THREADS - 1) / SGS_SIM_THREADS * 65025ll * 64 < (1ll << 32), "a wave's squared differences fit 32 bits");

// sgs_similarity_row (include/sage_gs.h) as the kernels update it: six 64-bit sums, then the two counts.
struct SimRow {
    unsigned long long sums[6];            // ssim_q[3] (two's complement), sse[3]
    unsigned long long n_windows, n_pixels;
};
static_assert(sizeof(SimRow) == 64, "sgs_similarity_row is 64 bytes");

struct SimJob {
    const float* rgb;                      // n_frames frames, rgb_stride floats apart
    const unsigned char* target;           // target_stride bytes apart (0: one target)
    SimRow* rows;                          // [n_frames]
    long long rgb_stride, target_stride;
    int W, H, n_frames, tiles_x;
};

// k_pack_rgba8's level of one channel.
__device__ __forceinline__ unsigned sim_level(float x) {
    const float c = fminf(fmaxf(x, 0.f), 1.f);
    return (unsigned)(c * 255.0f + 0.5f);
}

// Tap t of the 1-D window (constant after unrolling).
__device__ __forceinline__ unsigned sim_tap(int t) {
    constexpr unsigned w[SGS_SIM_TAPS] = {2, 16, 74, 224, 436, 544, 436, 224, 74, 16, 2};
    return w[t];
}

// acc + w * v in 64 bits (one v_mad_u64_u32).
__device__ __forceinline__ unsigned long long sim_mad64(unsigned long long acc, unsigned w, unsigned v) {
    return acc + (unsigned long long)w * v;
}

// q of one window and channel from its moments.
__device__ __forceinline__ long long sim_q(unsigned A, unsigned B, unsigned long long Cxx, unsigned long long Cyy, unsigned long long Cxy) {
    const long long c1 = SGS_SIM_C1, c2 = SGS_SIM_C2;
    const long long AB = (long long)((unsigned long long)A * B), AA = (long long)((unsigned long long)A * A), BB = (long long)((unsigned long long)B * B);
    const long long n1 = 2 * AB + c1;
    const long long d1 = AA + BB + c1;
    const long long n2 = 2 * ((long long)(Cxy << SGS_SIM_T_BITS) - AB) + c2;
    const long long d2 = ((long long)(Cxx << SGS_SIM_T_BITS) - AA) + ((long long)(Cyy << SGS_SIM_T_BITS) - BB) + c2;
    const double s = ((double)n1 * (double)n2) / ((double)d1 * (double)d2);
    const double v = s * 1073741824.0 + 0.5;
    return (long long)floor(v);
}

// Every frame's row: the counts, and zeros to add to.
__global__ __launch_bounds__(SGS_SIM_THREADS) void k_sim_clear(SimJob J) {
    const long long step = (long long)gridDim.x * SGS_SIM_THREADS;
    for (long long f = (long long)blockIdx.x * SGS_SIM_THREADS + threadIdx.x; f < J.n_frames; f += step) {
        SimRow e;
        for (int k = 0; k < 6; ++k) e.sums[k] = 0;
        e.n_windows = (unsigned long long)(J.W - (SGS_SIM_TAPS - 1)) * (unsigned long long)(J.H - (SGS_SIM_TAPS - 1));
        e.n_pixels = (unsigned long long)J.W * (unsigned long long)J.H;
        J.rows[f] = e;
    }
}

__global__ __launch_bounds__(SGS_SIM_THREADS) void k_sim_reduce(SimJob J) {
    __shared__ unsigned short s_xy[3][SGS_SIM_IN_H][SGS_SIM_IN_W + 2];           // x | y << 8 (rows padded to whole words)
    __shared__ unsigned s_h[5][SGS_SIM_IN_H][SGS_SIM_TILE_W];                    // A, B, Cxx, Cyy, Cxy along x
    __shared__ unsigned long long s_acc[6];
    const int tid = (int)threadIdx.x;
    const long long f = blockIdx.y;
    const int nwx = J.W - (SGS_SIM_TAPS - 1), nwy = J.H - (SGS_SIM_TAPS - 1);     // windows across, down
    const int ty = (int)(blockIdx.x / (unsigned)J.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)J.tiles_x);
    const int x0 = tx * SGS_SIM_TILE_W, y0 = ty * SGS_SIM_TILE_H;
    const bool last_x = x0 + SGS_SIM_TILE_W >= nwx, last_y = y0 + SGS_SIM_TILE_H >= nwy;
    const float* rgb = J.rgb + f * J.rgb_stride;
    const unsigned char* tgt = J.target + f * J.target_stride;

    if (tid < 6) s_acc[tid] = 0;

    // 1. the tile's pixels, once; the squared differences of the pixels it owns
    unsigned e0 = 0, e1 = 0, e2 = 0;
    for (int i = tid; i < SGS_SIM_IN_H * SGS_SIM_IN_W * 3; i += SGS_SIM_THREADS) {
        const int ly = i / (SGS_SIM_IN_W * 3), k = i - ly * (SGS_SIM_IN_W * 3);
        const int lx = k / 3, c = k - lx * 3;
        const int px = x0 + lx;
        const int py = y0 + ly;
        const bool in = px < J.W && py < J.H;
        unsigned x = 0, y = 0;
        if (in) {
            const long long at = ((long long)py * J.W + px) * 3 + c;
            x = sim_level(rgb[at]);
            y = tgt[at];
        }
        s_xy[c][ly][lx] = (unsigned short)(x | (y << 8));
        const bool owned = in && (lx < SGS_SIM_TILE_W || last_x) && (ly < SGS_SIM_TILE_H || last_y);
        const int d = (int)x - (int)y;
        const unsigned d2 = owned ? (unsigned)(d * d) : 0u;
        e0 += c == 0 ? d2 : 0u; e1 += c == 1 ? d2 : 0u; e2 += c == 2 ? d2 : 0u;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { e0 += __shfl_xor(e0, m); e1 += __shfl_xor(e1, m); e2 += __shfl_xor(e2, m); }
    __syncthreads();
    if ((tid & 63) == 0) {
        atomicAdd(&s_acc[3], (unsigned long long)e0); atomicAdd(&s_acc[4], (unsigned long long)e1); atomicAdd(&s_acc[5], (unsigned long long)e2);
    }

    const int col = tid & (SGS_SIM_TILE_W - 1), row0 = tid / SGS_SIM_TILE_W * SGS_SIM_ROWS;
    for (int c = 0; c < 3; ++c) {
        // 2. the five moments along x
        for (int i = tid; i < SGS_SIM_IN_H * SGS_SIM_TILE_W; i += SGS_SIM_THREADS) {
            const int ly = i / SGS_SIM_TILE_W, lx = i & (SGS_SIM_TILE_W - 1);
            unsigned a = 0, b = 0, xx = 0, yy = 0, xy = 0;
#pragma unroll
            for (int t = 0; t < SGS_SIM_TAPS; ++t) {
                const unsigned p = s_xy[c][ly][lx + t];
                const unsigned x = p & 255u, y = p >> 8, w = sim_tap(t);
                const unsigned wx = w * x, wy = w * y;
                a += wx; b += wy; xx += wx * x; yy += wy * y; xy += wx * y;
            }
            s_h[0][ly][lx] = a; s_h[1][ly][lx] = b; s_h[2][ly][lx] = xx; s_h[3][ly][lx] = yy; s_h[4][ly][lx] = xy;
        }
        __syncthreads();

        // 3. along y in registers, q per window
        unsigned A[SGS_SIM_ROWS], B[SGS_SIM_ROWS];
        unsigned long long XX[SGS_SIM_ROWS], YY[SGS_SIM_ROWS], XY[SGS_SIM_ROWS];
#pragma unroll
        for (int j = 0; j < SGS_SIM_ROWS; ++j) { A[j] = 0; B[j] = 0; XX[j] = 0; YY[j] = 0; XY[j] = 0; }
#pragma unroll
        for (int r = 0; r < SGS_SIM_ROWS + SGS_SIM_TAPS - 1; ++r) {
            const unsigned a = s_h[0][row0 + r][col], b = s_h[1][row0 + r][col];
            const unsigned xx = s_h[2][row0 + r][col], yy = s_h[3][row0 + r][col], xy = s_h[4][row0 + r][col];
#pragma unroll
            for (int j = 0; j < SGS_SIM_ROWS; ++j) {
                const int t = r - j;
                if (t < 0 || t >= SGS_SIM_TAPS) continue;
                const unsigned w = sim_tap(t);
                A[j] += w * a; B[j] += w * b;
                XX[j] = sim_mad64(XX[j], w, xx); YY[j] = sim_mad64(YY[j], w, yy); XY[j] = sim_mad64(XY[j], w, xy);
            }
        }
        long long q = 0;
#pragma unroll
        for (int j = 0; j < SGS_SIM_ROWS; ++j)
            if (x0 + col < nwx && y0 + row0 + j < nwy) q += sim_q(A[j], B[j], XX[j], YY[j], XY[j]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m);
        if ((tid & 63) == 0) atomicAdd(&s_acc[c], (unsigned long long)q);
        __syncthreads();                   // s_h is free again; after the last channel, s_acc is complete
    }

    // 4. one set of six 64-bit atomics per workgroup
    if (tid < 6) atomicAdd(&J.rows[f].sums[tid], s_acc[tid]);
}

}  // namespace sgs
