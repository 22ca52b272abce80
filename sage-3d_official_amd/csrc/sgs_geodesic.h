// sgs_geodesic.h — gfx950 kernels of the geodesic distance field and its shortest paths (sgs_geodesic_field, sgs_geodesic_path,
// include/sage_gs.h).
//
// How far a cell of a blocked grid is from the nearest seed (goal) when walls have to be walked round: the cheapest 8-connected walk
// over cells that are not blocked, a straight step costing 1 and a diagonal step sqrt(2); a diagonal step needs only its two end
// cells free (it may cut a corner, as the reference's astar_pixel does).  What the reference's trajectory generator computes with one
// host A* per (start, goal) pair; here one field from a goal answers every start of the map, and a batch of goals on one map is one
// call.
//
// A cost is the integer pair (a, b) = (straight steps, diagonal steps) and stands for a + b sqrt(2).  Two costs are compared exactly
// (geodesic_less): sqrt(2) is irrational, so two different pairs never cost the same, the cheapest pair of a cell is unique even where
// the walk is not, and no float decides an ordering.  The field is therefore the unique fixed point of the relaxation
//     d(c) = min(d(c), min over free neighbours n of d(n) + step(n, c)),  d(seed) = (0, 0),
// and its bits depend on the map and the seeds alone — not on the schedule, the tiling, the batch or how many rounds a call ran.
//
// Launches, all stream-ordered; no grid-wide barrier, no spinning, no cooperative launch:
//   k_geo_fill     dist <- NONE, the dirty flags and the blocked-seed counters of `state` <- 0
//   k_geo_put      up to SGS_GEO_PUT_WORDS words of a small host table (field_map), carried in the kernel's arguments, into `state`
//   k_geo_seed     up to SGS_GEO_SEEDS_PER_LAUNCH seeds, carried in the kernel's arguments: a free seed cell <- (0, 0), its tile and the tiles whose
//                  halo holds it dirty; a blocked one is counted
//   k_geo_relax    one launch per tile colour (tx & 1, ty & 1), four per round.  A workgroup owns one tile of SGS_GEO_TILE^2 cells of
//                  one field: not dirty, it exits at once; else it loads the tile and a one-cell halo (corners included) into LDS,
//                  relaxes until nothing in the workgroup changes, writes the cells that got smaller back, and marks dirty the
//                  neighbouring tiles (up to eight, the diagonal one included) whose halo holds a border cell that got smaller
//   k_geo_status   per field: the tiles still dirty and the seeds ignored, into `status`
//   k_geo_path     a thread owns a query: it walks downhill to a seed
//
// A round is race-free by construction.  The eight neighbours of a tile all have another colour than the tile, and two tiles of one
// colour lie at least a whole tile apart: within one launch a workgroup writes the cells and the dirty flag of its own tile only, and
// reads its own tile and a halo whose cells belong to tiles that do not run.  The dirty flags of tiles that do not run are only ever
// set (atomicOr); the flag of a tile that runs is read, then cleared, by that tile's workgroup alone.
//
// The local solve is a Jacobi iteration on LDS: every cell's candidate is computed from the values of the sweep before (barrier),
// then stored (barrier).  After k sweeps every cell whose cheapest walk from the halo or a seed stays inside the tile for at most k
// steps is final, so TILE^2 + 1 sweeps always suffice; the loop is cut at SGS_GEO_MAX_SWEEPS regardless, the tile staying dirty, so that
// a workgroup ends whatever it is given.  Cells outside the grid and blocked cells hold NONE and are never relaxed, so a neighbour's NONE is the only
// test a candidate needs.
#pragma once
#include "sgs_common.h"

#define SGS_GEO_TILE 32
#define SGS_GEO_THREADS 256
#define SGS_GEO_CELLS_PER_THREAD (SGS_GEO_TILE * SGS_GEO_TILE / SGS_GEO_THREADS)
#define SGS_GEO_HALO (SGS_GEO_TILE + 2)
#define SGS_GEO_MAX_SWEEPS (SGS_GEO_TILE * SGS_GEO_TILE + 2)   // of a local solve: a walk inside a tile has at most TILE^2 cells
#define SGS_GEO_MAX_N 4096
#define SGS_GEO_MAX_FIELDS 65535                    // gridDim.z
#define SGS_GEO_NONE 0xFFFFFFFFu
#define SGS_GEO_NONE2 0xFFFFFFFFFFFFFFFFull         // a pair: a in the low word, b in the high word
#define SGS_GEO_SRC_MASK8 0
#define SGS_GEO_SRC_D2 1
#define SGS_GEO_PUT_WORDS 128
#define SGS_GEO_SEEDS_PER_LAUNCH 64
#define SGS_GEO_PATH_MAX_FIELDS 512                 // sgs_geodesic_path carries field_map in its kernel's arguments

namespace sgs {

struct GeodesicJob {
    const void* src;                       // n_maps maps, stride elements apart: uint8 [ny][nx] or uint32 [ny][nx]
    unsigned long long* dist;              // [n_fields][ny][nx] pairs
    unsigned* state;                       // [n_fields] field_map, [n_fields] blocked seeds, [n_fields][tiles_y][tiles_x] dirty flags
    long long stride;
    int nx, ny, n_fields, kind;
    int tiles_x, tiles_y;
    int colour_x, colour_y;                // k_geo_relax: the tiles of this launch
    unsigned max_d2;
};

__device__ __forceinline__ const unsigned* geodesic_field_map(const GeodesicJob& J) { return J.state; }
__device__ __forceinline__ unsigned* geodesic_blocked_seeds(const GeodesicJob& J) { return J.state + J.n_fields; }
__device__ __forceinline__ unsigned* geodesic_flags(const GeodesicJob& J, int f) {
    return J.state + 2ll * J.n_fields + (long long)f * J.tiles_x * J.tiles_y;
}

// Whether cell (i, j) of map m is blocked.
__device__ __forceinline__ bool geodesic_blocked(const void* src, int kind, long long stride, unsigned max_d2, int nx, long long m, int j, int i) {
    const long long cell = (long long)j * nx + i;
    if (kind == SGS_GEO_SRC_MASK8) return static_cast<const unsigned char*>(src)[m * stride + cell] != 0;
    return static_cast<const unsigned*>(src)[m * stride + cell] <= max_d2;
}

// a1 + b1 sqrt(2) < a2 + b2 sqrt(2), exactly: with p = a1 - a2 and q = b2 - b1 it is p < q sqrt(2), decided by the signs and by p^2
// against 2 q^2 in 64-bit integers (|p|, |q| <= 4096^2: the squares stay below 2^49).  NONE is larger than every cost.
__device__ __forceinline__ bool geodesic_less(unsigned long long x, unsigned long long y) {
    if (x == SGS_GEO_NONE2) return false;
    if (y == SGS_GEO_NONE2) return true;
    const long long p = (long long)(unsigned)x - (long long)(unsigned)y;
    const long long q = (long long)(unsigned)(y >> 32) - (long long)(unsigned)(x >> 32);
    if (p <= 0 && q >= 0) return p != 0 || q != 0;
    if (p >= 0 && q <= 0) return false;
    if (p > 0) return p * p < 2 * q * q;                                           // q > 0
    return p * p > 2 * q * q;                                                      // p < 0, q < 0
}

__global__ __launch_bounds__(SGS_GEO_THREADS) void k_geo_fill(unsigned long long* dist, long long pairs, unsigned* zero, long long zero_words) {
    const long long step = (long long)gridDim.x * SGS_GEO_THREADS;
    const long long t = (long long)blockIdx.x * SGS_GEO_THREADS + threadIdx.x;
    for (long long i = t; i < pairs; i += step) dist[i] = SGS_GEO_NONE2;
    for (long long i = t; i < zero_words; i += step) zero[i] = 0;
}

struct GeodesicWords { unsigned w[SGS_GEO_PUT_WORDS]; };

__global__ __launch_bounds__(SGS_GEO_PUT_WORDS) void k_geo_put(unsigned* dst, GeodesicWords W, int n) {
    const int t = (int)threadIdx.x;
    if (t < n) dst[t] = W.w[t];
}

struct GeodesicSeeds { int s[SGS_GEO_SEEDS_PER_LAUNCH][3]; };

__global__ __launch_bounds__(SGS_GEO_SEEDS_PER_LAUNCH) void k_geo_seed(GeodesicJob J, GeodesicSeeds S, int n) {
    const int t = (int)threadIdx.x;
    if (t >= n) return;
    const int f = S.s[t][0], i = S.s[t][1], j = S.s[t][2];                         // (the host has checked all three)
    const long long m = geodesic_field_map(J)[f];
    if (geodesic_blocked(J.src, J.kind, J.stride, J.max_d2, J.nx, m, j, i)) {
        atomicAdd(&geodesic_blocked_seeds(J)[f], 1u);
        return;
    }
    J.dist[((long long)f * J.ny + j) * J.nx + i] = 0ull;
    // its tile is dirty, and so is every tile whose halo holds the seed: the seed's own tile may have nothing to relax (a tile of one cell)
    const int tx = i / SGS_GEO_TILE, ty = j / SGS_GEO_TILE, lx = i - tx * SGS_GEO_TILE, ly = j - ty * SGS_GEO_TILE;
    const int ex = lx == 0 ? -1 : lx == SGS_GEO_TILE - 1 ? 1 : 0, ey = ly == 0 ? -1 : ly == SGS_GEO_TILE - 1 ? 1 : 0;
    unsigned* flags = geodesic_flags(J, f);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            if ((dx != 0 && dx != ex) || (dy != 0 && dy != ey)) continue;
            const int nx_t = tx + dx, ny_t = ty + dy;
            if (nx_t >= 0 && nx_t < J.tiles_x && ny_t >= 0 && ny_t < J.tiles_y) atomicOr(&flags[ny_t * J.tiles_x + nx_t], 1u);
        }
}

__global__ __launch_bounds__(SGS_GEO_THREADS) void k_geo_relax(GeodesicJob J) {
    __shared__ unsigned long long s_d[SGS_GEO_HALO * SGS_GEO_HALO];
    __shared__ unsigned s_changed[2];
    __shared__ unsigned s_mark[9];
    const int tid = (int)threadIdx.x;
    const int tx = 2 * (int)blockIdx.x + J.colour_x, ty = 2 * (int)blockIdx.y + J.colour_y, f = (int)blockIdx.z;
    unsigned* flags = geodesic_flags(J, f);
    const int tile = ty * J.tiles_x + tx;
    if (flags[tile] == 0) return;                                                  // (workgroup-uniform: nobody writes this flag in this launch)
    const long long m = geodesic_field_map(J)[f];
    unsigned long long* dist = J.dist + (long long)f * J.ny * J.nx;
    const int x0 = tx * SGS_GEO_TILE, y0 = ty * SGS_GEO_TILE;

    // 1. the tile and its halo, corners included; a cell outside the grid is NONE
    for (int e = tid; e < SGS_GEO_HALO * SGS_GEO_HALO; e += SGS_GEO_THREADS) {
        const int hy = e / SGS_GEO_HALO, hx = e - hy * SGS_GEO_HALO;
        const int gx = x0 + hx - 1, gy = y0 + hy - 1;
        const bool inside = gx >= 0 && gx < J.nx && gy >= 0 && gy < J.ny;
        s_d[e] = inside ? dist[(long long)gy * J.nx + gx] : SGS_GEO_NONE2;
    }
    if (tid < 9) s_mark[tid] = 0;
    if (tid < 2) s_changed[tid] = 0;
    // the cells of this thread: free or not (a cell of a partial tile beyond the grid's edge is not), and what they held
    bool is_free[SGS_GEO_CELLS_PER_THREAD];
    for (int k = 0; k < SGS_GEO_CELLS_PER_THREAD; ++k) {
        const int c = tid + k * SGS_GEO_THREADS, ly = c / SGS_GEO_TILE, lx = c - ly * SGS_GEO_TILE;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool inside = gx < J.nx && gy < J.ny;
        is_free[k] = inside && !geodesic_blocked(J.src, J.kind, J.stride, J.max_d2, J.nx, m, gy, gx);
    }
    __syncthreads();
    if (tid == 0) flags[tile] = 0;
    unsigned long long first[SGS_GEO_CELLS_PER_THREAD], next[SGS_GEO_CELLS_PER_THREAD];
    for (int k = 0; k < SGS_GEO_CELLS_PER_THREAD; ++k) {
        const int c = tid + k * SGS_GEO_THREADS, ly = c / SGS_GEO_TILE, lx = c - ly * SGS_GEO_TILE;
        first[k] = s_d[(ly + 1) * SGS_GEO_HALO + lx + 1];
    }

    // 2. relax until nothing in the workgroup changes: candidates from the sweep before, barrier, stores, barrier
    for (unsigned sweep = 0;; ++sweep) {
        bool changed = false;
        for (int k = 0; k < SGS_GEO_CELLS_PER_THREAD; ++k) {
            const int c = tid + k * SGS_GEO_THREADS, ly = c / SGS_GEO_TILE, lx = c - ly * SGS_GEO_TILE;
            const int at = (ly + 1) * SGS_GEO_HALO + lx + 1;
            unsigned long long best = s_d[at];
            if (is_free[k]) {
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dx == 0 && dy == 0) continue;
                        const unsigned long long v = s_d[at + dy * SGS_GEO_HALO + dx];
                        if (v == SGS_GEO_NONE2) continue;
                        const unsigned long long cand = v + ((dx != 0 && dy != 0) ? (1ull << 32) : 1ull);
                        if (geodesic_less(cand, best)) { best = cand; changed = true; }
                    }
            }
            next[k] = best;
        }
        __syncthreads();
        if (changed) {
            for (int k = 0; k < SGS_GEO_CELLS_PER_THREAD; ++k) {
                const int c = tid + k * SGS_GEO_THREADS, ly = c / SGS_GEO_TILE, lx = c - ly * SGS_GEO_TILE;
                s_d[(ly + 1) * SGS_GEO_HALO + lx + 1] = next[k];
            }
            s_changed[sweep & 1] = 1;
        }
        if (tid == 0) s_changed[(sweep + 1) & 1] = 0;
        __syncthreads();
        if (!s_changed[sweep & 1]) break;
        if (sweep == SGS_GEO_MAX_SWEEPS) {                                         // (never with these kernels; a workgroup ends whatever it is given)
            if (tid == 0) atomicOr(&flags[tile], 1u);
            break;
        }
    }

    // 3. the cells that got smaller go back; a border cell among them makes the tiles dirty whose halo holds it
    for (int k = 0; k < SGS_GEO_CELLS_PER_THREAD; ++k) {
        const int c = tid + k * SGS_GEO_THREADS, ly = c / SGS_GEO_TILE, lx = c - ly * SGS_GEO_TILE;
        if (!is_free[k] || next[k] == first[k]) continue;
        dist[(long long)(y0 + ly) * J.nx + x0 + lx] = next[k];
        const int ex = lx == 0 ? -1 : lx == SGS_GEO_TILE - 1 ? 1 : 0, ey = ly == 0 ? -1 : ly == SGS_GEO_TILE - 1 ? 1 : 0;
        if (ex) s_mark[4 + ex] = 1;
        if (ey) s_mark[4 + 3 * ey] = 1;
        if (ex && ey) s_mark[4 + 3 * ey + ex] = 1;
    }
    __syncthreads();
    if (tid < 9 && tid != 4 && s_mark[tid]) {
        const int nx_t = tx + tid % 3 - 1, ny_t = ty + tid / 3 - 1;
        if (nx_t >= 0 && nx_t < J.tiles_x && ny_t >= 0 && ny_t < J.tiles_y) atomicOr(&flags[ny_t * J.tiles_x + nx_t], 1u);
    }
}

__global__ __launch_bounds__(SGS_GEO_THREADS) void k_geo_status(GeodesicJob J, unsigned* status) {
    __shared__ unsigned s_dirty;
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x;
    if (tid == 0) s_dirty = 0;
    __syncthreads();
    const unsigned* flags = geodesic_flags(J, f);
    unsigned n = 0;
    for (int t = tid; t < J.tiles_x * J.tiles_y; t += SGS_GEO_THREADS) n += flags[t] != 0 ? 1u : 0u;
    if (n) atomicAdd(&s_dirty, n);
    __syncthreads();
    if (tid == 0) {
        status[2 * f] = s_dirty;
        status[2 * f + 1] = geodesic_blocked_seeds(J)[f];
    }
}

// ---- sgs_geodesic_path --------------------------------------------------------------------------------------------------------------
struct GeodesicPathJob {
    const void* src;
    const unsigned long long* dist;
    const int* queries;                    // [n][3]: field, i, j
    int* cells;                            // [n][max_len][2]: i, j
    unsigned* info;                        // [n][2]: cells written, status
    long long stride;
    int nx, ny, n_fields, kind, n, max_len;
    unsigned max_d2;
    int field_map[SGS_GEO_PATH_MAX_FIELDS];
};

__global__ __launch_bounds__(SGS_GEO_THREADS) void k_geo_path(GeodesicPathJob Q) {
    const int k = (int)blockIdx.x * SGS_GEO_THREADS + (int)threadIdx.x;
    if (k >= Q.n) return;
    const int f = Q.queries[3 * k];
    int i = Q.queries[3 * k + 1], j = Q.queries[3 * k + 2];
    unsigned written = 0, status = 0;
    if (f < 0 || f >= Q.n_fields || i < 0 || i >= Q.nx || j < 0 || j >= Q.ny) status = 3;
    else {
        const long long m = Q.field_map[f];
        const unsigned long long* dist = Q.dist + (long long)f * Q.ny * Q.nx;
        unsigned long long cur = dist[(long long)j * Q.nx + i];
        if (cur == SGS_GEO_NONE2 || geodesic_blocked(Q.src, Q.kind, Q.stride, Q.max_d2, Q.nx, m, j, i)) status = 1;
        else {
            int* out = Q.cells + 2ll * k * Q.max_len;
            const unsigned long long steps = (cur & 0xFFFFFFFFull) + (cur >> 32);    // the walk has steps + 1 cells
            const int di[8] = {-1, 1, 0, 0, -1, -1, 1, 1}, dj[8] = {0, 0, -1, 1, -1, 1, -1, 1};
            for (unsigned long long s = 0;; ++s) {
                if (written == (unsigned)Q.max_len) { status = 2; break; }
                out[2 * written] = i;
                out[2 * written + 1] = j;
                ++written;
                if (s == steps) break;
                int d = 0;
                for (; d < 8; ++d) {
                    const int ni = i + di[d], nj = j + dj[d];
                    if (ni < 0 || ni >= Q.nx || nj < 0 || nj >= Q.ny) continue;
                    if (geodesic_blocked(Q.src, Q.kind, Q.stride, Q.max_d2, Q.nx, m, nj, ni)) continue;
                    const unsigned long long v = dist[(long long)nj * Q.nx + ni];
                    if (v == SGS_GEO_NONE2) continue;
                    if (v + (d < 4 ? 1ull : (1ull << 32)) == cur) { i = ni; j = nj; cur = v; break; }
                }
                if (d == 8) { status = 4; break; }                                 // no downhill neighbour: the field is not final
            }
        }
    }
    Q.info[2 * k] = written;
    Q.info[2 * k + 1] = status;
}

}  // namespace sgs
