// sgs_endpoints.h — gfx950 kernels of the item endpoints (sgs_endpoints, include/sage_gs.h).
//
// For an item — a list of cells, duplicates allowed — the free cell nearest to its boundary on the side that faces a target: what the
// reference's get_nearest_free_pixel_on_side finds with a breadth-first search over Python sets.  That search starts from the boundary
// B (the item's cells with a 4-neighbour outside the item), is 4-connected and walks through obstacles, so a cell's level is its L1
// distance to B: a capped L1 distance transform per item, then a reduction per query.
//
// An item's WINDOW is its tight box grown by max_dist and clipped to the grid; every cell within max_dist of B lies in it, and so does
// an L1-shortest walk to it.  The windows lie end to end in `work`, one byte per cell, behind a header of one uint64 offset per item.
// Launches, all stream-ordered; kernel boundaries are the only synchronisation between workgroups, no workgroup waits for another,
// and every loop has its bound in its header:
//   k_ep_items     a workgroup per item: its CSR slice -> n, flags, sums of x and y, the box, the centroid pixel (half to even)
//   k_ep_scan      one workgroup: the exclusive scan of the windows' sizes -> the header; counters [2] (flagged items), [3] (bytes of
//                  work needed) and zeroes into [0], [1].  Every later kernel returns at once when [3] > work_bytes.
//   k_ep_clear     zeroes the windows
//   k_ep_mark      a thread per CSR entry: the member's byte <- 1 (duplicates store the same value)
//   k_ep_boundary  a wave per 64 cells of a window row: a member with a 4-neighbour that is no member (outside the window is outside
//                  the box: no member) <- 2.  "Member" is byte != 0 before and after, so the neighbours' reads do not care which
//                  they see.  The ballot's popcount -> the row's boundary count.
//   k_ep_rows      a wave per window row: the ballot word of the boundary lanes of every 64-cell segment (lane s keeps word s; a row
//                  has at most 64), then per segment the distance to the nearest set bit left and right from __clzll / __ffsll on
//                  the word and its two neighbours — exact up to 64, which is enough because max_dist <= 63 — capped at 255.  A row
//                  belongs to one wave, which reads all of it before it writes.
//   k_ep_cols      a lane per window column: d = min(d, above + 1) downwards, then upwards; bytes above max_dist <- 255.  After it a
//                  byte is the exact L1 distance to B, or 255.
//   k_ep_query     a workgroup per query: over its item's window the triple (least d, cells at that d, least raster index at that d)
//                  among the cells that are free and, with a target, in the half-plane — the key d << 24 | index and a count, by
//                  lane, by wave (__shfl_xor), through LDS, one store.  The half-plane is exact in int64:
//                  (n x - Sx)(n tx - Sx) + (n y - Sy)(n ty - Sy) >= 0; n <= 2^19 and x < 2^12 keep a factor below 2^31.
// Everything is an integer minimum, count or sum: the output is a function of the inputs alone.
#pragma once
#include "sgs_common.h"

#define SGS_EP_THREADS 256
#define SGS_EP_WAVES (SGS_EP_THREADS / 64)
#define SGS_EP_TILE 64                                            // cells of one ballot word
#define SGS_EP_MAX_N 4096
#define SGS_EP_MAX_ITEMS 65535
#define SGS_EP_MAX_DIST 63
#define SGS_EP_MAX_ENTRIES (1u << 19)
#define SGS_EP_FAR 255u
#define SGS_EP_SRC_MASK8 0
#define SGS_EP_SRC_D2 1
#define SGS_EP_ITEM_EMPTY 1u
#define SGS_EP_ITEM_BAD_CELL 2u
#define SGS_EP_ITEM_TOO_LONG 4u
#define SGS_EP_QUERY_TOWARDS 1u
#define SGS_EP_NO_KEY 0xFFFFFFFFu

namespace sgs {

// sgs_endpoints_item, sgs_endpoints_query and sgs_endpoints_answer (include/sage_gs.h) as the kernels see them.
struct EpItem {
    unsigned n, flags;
    int x_min, y_min, x_end, y_end;
    int cx, cy;
    unsigned boundary, reserved;
    unsigned long long sum_x, sum_y;
};
static_assert(sizeof(EpItem) == 56, "sgs_endpoints_item is 56 bytes");
struct EpQuery { int item, tx, ty; unsigned flags; };
struct EpAnswer { int x, y, d, n_at_d; };

struct EpJob {
    const void* src;                       // uint8 [ny][nx] or uint32 [ny][nx]
    const unsigned* offsets;               // [n_items + 1]
    const int* cells;                      // raster indices
    const EpQuery* queries;
    unsigned long long* win_off;           // work: [n_items], a window's first byte in `field`
    unsigned char* field;                  // work behind the header
    EpItem* items;
    EpAnswer* answers;
    unsigned long long* counts;            // [4]
    unsigned long long work_bytes;
    int nx, ny, n_items, n_queries, kind, max_dist, has_header;
    unsigned max_d2;
};

struct EpWin { int x0, y0, w, h; };

// The window of an item row: its box grown by max_dist, clipped; empty for a flagged item.
__device__ __forceinline__ EpWin ep_window(const EpJob& J, const EpItem& r) {
    EpWin W = {0, 0, 0, 0};
    if (r.flags != 0) return W;
    W.x0 = max(r.x_min - J.max_dist, 0); W.y0 = max(r.y_min - J.max_dist, 0);
    W.w = min(r.x_end + J.max_dist, J.nx) - W.x0; W.h = min(r.y_end + J.max_dist, J.ny) - W.y0;
    return W;
}

__device__ __forceinline__ bool ep_fits(const EpJob& J) { return J.counts[3] <= J.work_bytes; }

// S / n rounded half to even, as int(round(mean)) rounds the exact quotient.
__device__ __forceinline__ int ep_round_half_even(unsigned long long s, unsigned long long n) {
    const unsigned long long q = s / n, r = s - q * n;
    if (2 * r > n) return (int)(q + 1);
    if (2 * r == n) return (int)(q + (q & 1ull));
    return (int)q;
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_items(EpJob J) {
    __shared__ unsigned long long s_sx[SGS_EP_WAVES], s_sy[SGS_EP_WAVES];
    __shared__ unsigned s_box[SGS_EP_WAVES][4], s_bad[SGS_EP_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = (int)blockIdx.x;
    const unsigned begin = J.offsets[item], end = J.offsets[item + 1];
    const unsigned n = end > begin ? end - begin : 0u;
    unsigned flags = n == 0 ? SGS_EP_ITEM_EMPTY : n > SGS_EP_MAX_ENTRIES ? SGS_EP_ITEM_TOO_LONG : 0u;
    const unsigned n_read = flags ? 0u : n;                                          // a flagged slice is not read
    const unsigned n_cells = (unsigned)J.nx * (unsigned)J.ny;
    unsigned long long sx = 0, sy = 0;
    unsigned x0 = 0x7FFFFFFFu, y0 = 0x7FFFFFFFu, x1 = 0, y1 = 0, bad = 0;
    for (unsigned e = (unsigned)tid; e < n_read; e += SGS_EP_THREADS) {
        const unsigned c = (unsigned)J.cells[begin + e];                             // a negative index is a large one
        if (c >= n_cells) { bad = 1; continue; }
        const unsigned y = c / (unsigned)J.nx, x = c - y * (unsigned)J.nx;
        sx += x; sy += y;
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1u); y1 = max(y1, y + 1u);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        sx += __shfl_xor(sx, m); sy += __shfl_xor(sy, m);
        x0 = min(x0, __shfl_xor(x0, m)); y0 = min(y0, __shfl_xor(y0, m));
        x1 = max(x1, __shfl_xor(x1, m)); y1 = max(y1, __shfl_xor(y1, m));
        bad |= __shfl_xor(bad, m);
    }
    if (lane == 0) { s_sx[wave] = sx; s_sy[wave] = sy; s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = x1; s_box[wave][3] = y1; s_bad[wave] = bad; }
    __syncthreads();
    if (tid != 0) return;
    for (int u = 1; u < SGS_EP_WAVES; ++u) {
        sx += s_sx[u]; sy += s_sy[u]; bad |= s_bad[u];
        x0 = min(x0, s_box[u][0]); y0 = min(y0, s_box[u][1]); x1 = max(x1, s_box[u][2]); y1 = max(y1, s_box[u][3]);
    }
    if (bad) flags |= SGS_EP_ITEM_BAD_CELL;
    EpItem r;
    r.n = n; r.flags = flags; r.boundary = 0; r.reserved = 0;
    if (flags) { r.x_min = 0x7FFFFFFF; r.y_min = 0x7FFFFFFF; r.x_end = 0; r.y_end = 0; r.cx = -1; r.cy = -1; r.sum_x = 0; r.sum_y = 0; }
    else {
        r.x_min = (int)x0; r.y_min = (int)y0; r.x_end = (int)x1; r.y_end = (int)y1; r.sum_x = sx; r.sum_y = sy;
        r.cx = ep_round_half_even(sx, n); r.cy = ep_round_half_even(sy, n);
    }
    J.items[item] = r;
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_scan(EpJob J) {
    __shared__ unsigned long long s_bytes[SGS_EP_THREADS];
    __shared__ unsigned s_flagged[SGS_EP_THREADS];
    const int tid = (int)threadIdx.x;
    const int per = (J.n_items + SGS_EP_THREADS - 1) / SGS_EP_THREADS;              // consecutive items of this thread
    const int i0 = min(tid * per, J.n_items), i1 = min(i0 + per, J.n_items);
    unsigned long long bytes = 0;
    unsigned flagged = 0;
    for (int i = i0; i < i1; ++i) {
        const EpWin W = ep_window(J, J.items[i]);
        bytes += (unsigned long long)W.w * (unsigned long long)W.h;
        flagged += J.items[i].flags != 0;
    }
    s_bytes[tid] = bytes; s_flagged[tid] = flagged;
    __syncthreads();
    unsigned long long base = 0;
    for (int u = 0; u < tid; ++u) base += s_bytes[u];
    if (J.has_header)
        for (int i = i0; i < i1; ++i) {
            const EpWin W = ep_window(J, J.items[i]);
            J.win_off[i] = base;
            base += (unsigned long long)W.w * (unsigned long long)W.h;
        }
    if (tid == SGS_EP_THREADS - 1) {
        unsigned long long total = 0;
        unsigned n_flagged = 0;
        for (int u = 0; u < SGS_EP_THREADS; ++u) { total += s_bytes[u]; n_flagged += s_flagged[u]; }
        J.counts[0] = 0; J.counts[1] = 0; J.counts[2] = n_flagged;
        J.counts[3] = 8ull * (unsigned long long)J.n_items + ((total + 7ull) & ~7ull);
    }
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_clear(EpJob J) {
    if (!ep_fits(J)) return;
    const unsigned long long words = (J.counts[3] - 8ull * (unsigned long long)J.n_items) / 8ull;
    unsigned long long* f = reinterpret_cast<unsigned long long*>(J.field);
    const unsigned long long step = (unsigned long long)gridDim.x * SGS_EP_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * SGS_EP_THREADS + threadIdx.x; i < words; i += step) f[i] = 0ull;
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_mark(EpJob J) {
    if (!ep_fits(J)) return;
    const int item = (int)blockIdx.y;
    const EpItem r = J.items[item];
    const EpWin W = ep_window(J, r);
    if (W.w == 0) return;
    unsigned char* f = J.field + J.win_off[item];
    const unsigned begin = J.offsets[item];
    const unsigned step = gridDim.x * SGS_EP_THREADS;
    for (unsigned e = blockIdx.x * SGS_EP_THREADS + threadIdx.x; e < r.n; e += step) {
        const int c = J.cells[begin + e];                                            // in the grid: the item is not flagged
        const int y = c / J.nx, x = c - y * J.nx;
        f[(y - W.y0) * W.w + (x - W.x0)] = 1;
    }
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_boundary(EpJob J) {
    if (!ep_fits(J)) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = (int)blockIdx.y;
    const EpWin W = ep_window(J, J.items[item]);
    if (W.w == 0) return;
    unsigned char* f = J.field + J.win_off[item];
    const int segs = (W.w + SGS_EP_TILE - 1) / SGS_EP_TILE, units = W.h * segs;
    unsigned found = 0;
    for (int u = (int)blockIdx.x * SGS_EP_WAVES + wave; u < units; u += (int)gridDim.x * SGS_EP_WAVES) {
        const int row = u / segs, lx = (u - row * segs) * SGS_EP_TILE + lane;
        bool is_boundary = false;
        if (lx < W.w && f[row * W.w + lx] != 0) {
            const bool left = lx > 0 && f[row * W.w + lx - 1] != 0, right = lx + 1 < W.w && f[row * W.w + lx + 1] != 0;
            const bool up = row > 0 && f[(row - 1) * W.w + lx] != 0, down = row + 1 < W.h && f[(row + 1) * W.w + lx] != 0;
            is_boundary = !(left && right && up && down);
            if (is_boundary) f[row * W.w + lx] = 2;
        }
        found += (unsigned)__popcll(__ballot(is_boundary));
    }
    if (lane == 0 && found) atomicAdd(&J.items[item].boundary, found);
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_rows(EpJob J) {
    if (!ep_fits(J)) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = (int)blockIdx.y;
    const EpWin W = ep_window(J, J.items[item]);
    if (W.w == 0) return;
    unsigned char* f = J.field + J.win_off[item];
    const int segs = (W.w + SGS_EP_TILE - 1) / SGS_EP_TILE;                         // <= 64: a lane per word
    for (int row = (int)blockIdx.x * SGS_EP_WAVES + wave; row < W.h; row += (int)gridDim.x * SGS_EP_WAVES) {
        unsigned char* line = f + row * W.w;
        unsigned long long mine = 0;
        for (int s = 0; s < segs; ++s) {
            const int lx = s * SGS_EP_TILE + lane;
            const unsigned long long word = __ballot(lx < W.w && line[lx] == 2);
            if (lane == s) mine = word;
        }
        for (int s = 0; s < segs; ++s) {
            const unsigned long long mid = __shfl(mine, s), l = __shfl(mine, max(s - 1, 0)), r = __shfl(mine, min(s + 1, segs - 1));
            const unsigned long long left = s > 0 ? l : 0ull, right = s + 1 < segs ? r : 0ull;
            const unsigned long long at_or_below = mid & (~0ull >> (63 - lane)), at_or_above = mid >> lane;
            unsigned d = SGS_EP_FAR;
            if (at_or_below) d = (unsigned)(lane - (63 - __clzll((long long)at_or_below)));
            else if (left) d = (unsigned)(lane + 1 + __clzll((long long)left));
            if (at_or_above) d = min(d, (unsigned)(__ffsll((long long)at_or_above) - 1));
            else if (right) d = min(d, (unsigned)(64 - lane + __ffsll((long long)right) - 1));
            const int lx = s * SGS_EP_TILE + lane;
            if (lx < W.w) line[lx] = (unsigned char)min(d, SGS_EP_FAR);
        }
    }
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_cols(EpJob J) {
    if (!ep_fits(J)) return;
    const int item = (int)blockIdx.y;
    const EpWin W = ep_window(J, J.items[item]);
    if (W.w == 0) return;
    unsigned char* f = J.field + J.win_off[item];
    for (int col = (int)(blockIdx.x * SGS_EP_THREADS + threadIdx.x); col < W.w; col += (int)gridDim.x * SGS_EP_THREADS) {
        unsigned above = SGS_EP_FAR;
        for (int y = 0; y < W.h; ++y) {
            const unsigned d = min((unsigned)f[y * W.w + col], min(above + 1u, SGS_EP_FAR));
            f[y * W.w + col] = (unsigned char)d;
            above = d;
        }
        unsigned below = SGS_EP_FAR;
        for (int y = W.h - 1; y >= 0; --y) {
            const unsigned d = min((unsigned)f[y * W.w + col], min(below + 1u, SGS_EP_FAR));
            f[y * W.w + col] = (unsigned char)(d <= (unsigned)J.max_dist ? d : SGS_EP_FAR);
            below = d;
        }
    }
}

__device__ __forceinline__ bool ep_free(const EpJob& J, unsigned cell) {
    return J.kind == SGS_EP_SRC_MASK8 ? static_cast<const unsigned char*>(J.src)[cell] == 0 : static_cast<const unsigned*>(J.src)[cell] > J.max_d2;
}

// (key, count) of two sets of candidates: the smaller d wins, equal d add their counts and keep the smaller index.
__device__ __forceinline__ void ep_merge(unsigned& key, unsigned& count, unsigned o_key, unsigned o_count) {
    const unsigned d = key >> 24, o_d = o_key >> 24;
    if (o_d < d) { key = o_key; count = o_count; }
    else if (o_d == d) { key = min(key, o_key); count += o_count; }
}

__global__ __launch_bounds__(SGS_EP_THREADS) void k_ep_query(EpJob J) {
    __shared__ unsigned s_key[SGS_EP_WAVES], s_count[SGS_EP_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EpQuery q = J.queries[blockIdx.x];
    const bool towards = (q.flags & SGS_EP_QUERY_TOWARDS) != 0;
    bool valid = ep_fits(J) && q.item >= 0 && q.item < J.n_items && (q.flags & ~SGS_EP_QUERY_TOWARDS) == 0;
    if (towards && (q.tx < 0 || q.tx >= J.nx || q.ty < 0 || q.ty >= J.ny)) valid = false;
    EpWin W = {0, 0, 0, 0};
    long long n = 0, sx = 0, sy = 0;
    const unsigned char* f = J.field;
    if (valid) {                                                                     // no index of an invalid query becomes an address
        const EpItem r = J.items[q.item];
        W = ep_window(J, r);
        n = r.n; sx = (long long)r.sum_x; sy = (long long)r.sum_y;
        if (W.w != 0) f += J.win_off[q.item];
    }
    const long long ax = n * q.tx - sx, ay = n * q.ty - sy;                          // n (target - centroid)
    unsigned key = SGS_EP_NO_KEY, count = 0;
    const int cells = W.w * W.h;
    for (int c = tid; c < cells; c += SGS_EP_THREADS) {
        const unsigned d = f[c];
        if (d == SGS_EP_FAR || d > (key >> 24)) continue;
        const int wy = c / W.w, x = W.x0 + c - wy * W.w, y = W.y0 + wy;
        const unsigned cell = (unsigned)y * (unsigned)J.nx + (unsigned)x;
        if (!ep_free(J, cell)) continue;
        if (towards && (n * x - sx) * ax + (n * y - sy) * ay < 0) continue;
        ep_merge(key, count, (d << 24) | cell, 1u);
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned o_key = __shfl_xor(key, m), o_count = __shfl_xor(count, m);
        ep_merge(key, count, o_key, o_count);
    }
    if (lane == 0) { s_key[wave] = key; s_count[wave] = count; }
    __syncthreads();
    if (tid != 0) return;
    for (int u = 1; u < SGS_EP_WAVES; ++u) ep_merge(key, count, s_key[u], s_count[u]);
    EpAnswer a = {-1, -1, -1, 0};
    if (key != SGS_EP_NO_KEY) {
        const unsigned cell = key & 0xFFFFFFu;
        a.y = (int)(cell / (unsigned)J.nx); a.x = (int)(cell - (unsigned)a.y * (unsigned)J.nx); a.d = (int)(key >> 24); a.n_at_d = (int)count;
    }
    J.answers[blockIdx.x] = a;
    atomicAdd(reinterpret_cast<unsigned*>(&J.counts[key != SGS_EP_NO_KEY ? 0 : 1]), 1u);      // the low word: fewer than 2^32 queries
}

}  // namespace sgs
