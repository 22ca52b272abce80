// sgs_regions.h — gfx950 kernels of the connected regions of a grid (sgs_regions_label, include/sage_gs.h).
//
// Which cells belong together: the classes of the set {lo <= v <= hi} under 4- or 8-connectivity, numbered 1, 2, ... by their least
// raster index j * nx + i (scipy.ndimage.label's numbering), with a row per region (area, box, first cell, sums of x and y) and four
// counters per map.  What the reference's semantic_map_builder.py computes with two scipy.ndimage.label calls per scene on the host.
//
// A region is represented by a forest over the cells: parent[c] <= c is a cell of c's region (a raster index), a root has
// parent[c] == c, a cell outside the set holds NONE.  Parents only ever DECREASE, from the first store to the last; everything below
// follows from that.  Launches, all stream-ordered; kernel boundaries are the only synchronisation between phases, no workgroup waits
// for another, and every loop has a bound in its header:
//   k_reg_clear    the empty row into every row of out_rows
//   k_reg_local    a workgroup per tile of SGS_REG_TILE^2 cells of one map: min-propagation with one pointer jump per sweep on LDS to the
//                  fixed point — every cell of a piece (the part of a region inside the tile) then holds the piece's least cell —, and
//                  parent <- that cell's raster index.  Cells of a partial tile beyond the map are outside the set.
//   k_reg_merge    a thread per cell on the low side of a tile border: it unites its cell with the (up to three) cells across the
//                  border.  The pass over horizontal borders takes every such pair, the diagonal ones through a tile corner included;
//                  the pass over vertical borders takes the pairs that stay inside one tile row.
//   k_reg_flatten  root[c] <- the root of c (it reads parent and writes root: nothing is read and written in one launch), and per
//                  chunk of SGS_REG_CHUNK cells the roots and the cells in the set
//   k_reg_scan     a workgroup per map: the exclusive scan of the chunks' root counts; counters [0] and [1]
//   k_reg_rank     a root's label = 1 + the roots before it in raster order = its chunk's base + the roots before it in the chunk;
//                  parent[root] <- label (the forest is no longer needed)
//   k_reg_labels   labels[c] <- parent[root[c]], 0 outside the set; root[c] <- 0: the array becomes area[label - 1]
//   k_reg_rows     k_obj_reduce's reduction (csrc/sgs_objects.h) over the labels: runs of one label within a wave in closed form, a
//                  table of SGS_REG_SLOTS labels per workgroup in LDS, then one set of integer atomics per (workgroup, label);
//                  area[label - 1] for every label, the row for labels <= max_regions
//   k_reg_largest  a workgroup per map: the largest area and the least label that has it; counters [2] and [3]
//
// The union (reg_unite) is lock-free: find both roots, and link the LARGER root to the smaller with atomicMin(&parent[larger],
// smaller).  If the value the atomic returns is `larger`, it was still a root and now is linked; otherwise somebody linked it first
// to `old` < larger, the atomicMin has stored min(old, smaller) — still a cell of the same region, still smaller than `larger` — and
// the pair (old, smaller) is united next.
//   Termination  parent[c] <= c always, and a find step moves to a strictly smaller index: at most `cells` steps.  A retry replaces
//                the larger root by something strictly smaller: the sum of the pair strictly decreases, at most 2 * cells retries.
//   Determinism  links only ever join cells of one region, and every adjacency is united by some thread, so the final forest has one
//                tree per region; a tree's root is smaller than all its cells and is one of them: the region's least raster index,
//                whatever the schedule.  Labels, rows and counters are functions of the roots alone.
//   Stale reads  a parent read late is a value the cell held earlier: a larger ancestor-to-be of the same region.  find then ends on
//                a cell that may no longer be a root; the atomicMin on it returns its current parent and the loop goes on from there.
// Inside k_reg_merge parents are read with agent-scope relaxed atomic loads and written with atomicMin alone, so a value comes from
// the coherent level whichever XCD the other workgroup runs on; across launches the kernel boundary orders everything.
#pragma once
#include "sgs_common.h"

#define SGS_REG_TILE 32
#define SGS_REG_THREADS 256
#define SGS_REG_CELLS_PER_THREAD (SGS_REG_TILE * SGS_REG_TILE / SGS_REG_THREADS)
#define SGS_REG_HALO (SGS_REG_TILE + 2)
#define SGS_REG_MAX_SWEEPS (SGS_REG_TILE * SGS_REG_TILE + 1)      // of a local solve: min-propagation alone is final after TILE^2 sweeps
#define SGS_REG_MAX_N 4096
#define SGS_REG_MAX_MAPS 65535                                     // gridDim.y / gridDim.z
#define SGS_REG_NONE 0xFFFFFFFFu
#define SGS_REG_SRC_MASK8 0
#define SGS_REG_SRC_D2 1
#define SGS_REG_PER_THREAD 4
#define SGS_REG_CHUNK (SGS_REG_THREADS * SGS_REG_PER_THREAD)       // cells per workgroup of k_reg_flatten, k_reg_rank, k_reg_labels
#define SGS_REG_WAVES (SGS_REG_THREADS / 64)
#define SGS_REG_ROW_PER_THREAD 8
#define SGS_REG_ROW_REGION (SGS_REG_THREADS * SGS_REG_ROW_PER_THREAD)   // cells per workgroup of k_reg_rows
#define SGS_REG_SLOT_BITS 7
#define SGS_REG_SLOTS (1 << SGS_REG_SLOT_BITS)
#define SGS_REG_HASH 0x9E3779B1u

namespace sgs {

// sgs_region_row (include/sage_gs.h) as the kernels update it: the int32 fields through their unsigned views.
struct RegRow {
    unsigned area;
    unsigned x_min, y_min, x_end, y_end;
    unsigned first;
    unsigned long long sum_x, sum_y;
};
static_assert(sizeof(RegRow) == 40, "sgs_region_row is 40 bytes");

struct RegionsJob {
    const void* src;                       // n_maps maps, stride elements apart: uint8 [ny][nx] or uint32 [ny][nx]
    unsigned* parent;                      // work: [n_maps][cells]; after k_reg_rank parent[root] is the root's label
    unsigned* root;                        // work: [n_maps][cells]; after k_reg_labels area[label - 1]
    unsigned* chunks;                      // work: [n_maps][n_chunks][2]: roots (after k_reg_scan: the roots before the chunk), cells in the set
    int* labels;                           // [n_maps][ny][nx]
    RegRow* rows;                          // [n_maps][max_regions], or nullptr
    unsigned* counts;                      // [n_maps][4]
    long long stride;
    int nx, ny, n_maps, kind, conn;
    int tiles_x, tiles_y, n_chunks, max_regions;
    unsigned lo, hi, cells;
};

__device__ __forceinline__ bool reg_in_set(const RegionsJob& J, long long m, long long cell) {
    const unsigned v = J.kind == SGS_REG_SRC_MASK8 ? (unsigned)static_cast<const unsigned char*>(J.src)[m * J.stride + cell]
                                                   : static_cast<const unsigned*>(J.src)[m * J.stride + cell];
    return J.lo <= v && v <= J.hi;
}

__device__ __forceinline__ unsigned reg_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x while other threads link roots: at most `cells` steps, each to a strictly smaller index.
__device__ __forceinline__ unsigned reg_find(const unsigned* parent, unsigned x, unsigned cells) {
    for (unsigned step = 0; step < cells; ++step) {
        const unsigned p = reg_load(&parent[x]);
        if (p == x) break;
        x = p;
    }
    return x;
}

__device__ __forceinline__ void reg_unite(unsigned* parent, unsigned a, unsigned b, unsigned cells) {
    for (unsigned retry = 0; retry < 2u * cells; ++retry) {
        a = reg_find(parent, a, cells);
        b = reg_find(parent, b, cells);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }                        // a is the larger root: it gets the parent
        const unsigned old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_clear(RegRow* rows, long long n_rows) {
    const long long step = (long long)gridDim.x * SGS_REG_THREADS;
    for (long long i = (long long)blockIdx.x * SGS_REG_THREADS + threadIdx.x; i < n_rows; i += step) {
        RegRow e;
        e.area = 0; e.x_min = 0x7FFFFFFFu; e.y_min = 0x7FFFFFFFu; e.x_end = 0; e.y_end = 0; e.first = SGS_REG_NONE; e.sum_x = 0; e.sum_y = 0;
        rows[i] = e;
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_local(RegionsJob J) {
    __shared__ unsigned s_lab[SGS_REG_HALO * SGS_REG_HALO];                        // a cell's label is a local index ly * TILE + lx; NONE outside the set
    __shared__ unsigned s_changed[2];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * SGS_REG_TILE, y0 = (int)blockIdx.y * SGS_REG_TILE;
    const long long m = blockIdx.z;
    for (int e = tid; e < SGS_REG_HALO * SGS_REG_HALO; e += SGS_REG_THREADS) s_lab[e] = SGS_REG_NONE;
    if (tid < 2) s_changed[tid] = 0;
    __syncthreads();
    bool in_set[SGS_REG_CELLS_PER_THREAD];
    unsigned next[SGS_REG_CELLS_PER_THREAD];
    for (int k = 0; k < SGS_REG_CELLS_PER_THREAD; ++k) {
        const int c = tid + k * SGS_REG_THREADS, ly = c / SGS_REG_TILE, lx = c - ly * SGS_REG_TILE;
        const int gx = x0 + lx, gy = y0 + ly;
        const bool inside = gx < J.nx && gy < J.ny;
        in_set[k] = inside && reg_in_set(J, m, (long long)gy * J.nx + gx);
        next[k] = in_set[k] ? (unsigned)c : SGS_REG_NONE;
        s_lab[(ly + 1) * SGS_REG_HALO + lx + 1] = next[k];
    }
    __syncthreads();
    // candidates from the sweep before, barrier, stores, barrier.  A label is a cell of the same piece, never larger than the cell:
    // the least neighbouring label, then that cell's own label (one pointer jump).  At the fixed point every cell of a piece holds
    // the piece's least cell.
    for (unsigned sweep = 0;; ++sweep) {
        bool changed = false;
        for (int k = 0; k < SGS_REG_CELLS_PER_THREAD; ++k) {
            if (!in_set[k]) continue;
            const int c = tid + k * SGS_REG_THREADS, ly = c / SGS_REG_TILE, lx = c - ly * SGS_REG_TILE;
            const int at = (ly + 1) * SGS_REG_HALO + lx + 1;
            unsigned best = s_lab[at];
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (dx != 0 && dy != 0 && J.conn == 4) continue;
                    best = min(best, s_lab[at + dy * SGS_REG_HALO + dx]);
                }
            const int by = (int)best / SGS_REG_TILE, bx = (int)best - by * SGS_REG_TILE;
            best = s_lab[(by + 1) * SGS_REG_HALO + bx + 1];
            if (best != next[k]) changed = true;
            next[k] = best;
        }
        __syncthreads();
        if (changed) {
            for (int k = 0; k < SGS_REG_CELLS_PER_THREAD; ++k) {
                const int c = tid + k * SGS_REG_THREADS, ly = c / SGS_REG_TILE, lx = c - ly * SGS_REG_TILE;
                s_lab[(ly + 1) * SGS_REG_HALO + lx + 1] = next[k];
            }
            s_changed[sweep & 1] = 1;
        }
        if (tid == 0) s_changed[(sweep + 1) & 1] = 0;
        __syncthreads();
        if (!s_changed[sweep & 1] || sweep == SGS_REG_MAX_SWEEPS) break;
    }
    unsigned* parent = J.parent + m * (long long)J.cells;
    for (int k = 0; k < SGS_REG_CELLS_PER_THREAD; ++k) {
        const int c = tid + k * SGS_REG_THREADS, ly = c / SGS_REG_TILE, lx = c - ly * SGS_REG_TILE;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= J.nx || gy >= J.ny) continue;
        const int ry = (int)next[k] / SGS_REG_TILE, rx = (int)next[k] - ry * SGS_REG_TILE;
        parent[(unsigned)gy * (unsigned)J.nx + (unsigned)gx] = in_set[k] ? (unsigned)(y0 + ry) * (unsigned)J.nx + (unsigned)(x0 + rx) : SGS_REG_NONE;
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_merge(RegionsJob J) {
    const long long m = blockIdx.y;
    unsigned* parent = J.parent + m * (long long)J.cells;
    const long long n_h = (long long)(J.tiles_y - 1) * J.nx, n_v = (long long)(J.tiles_x - 1) * J.ny;
    long long t = (long long)blockIdx.x * SGS_REG_THREADS + threadIdx.x;
    if (t < n_h) {
        // the cell above a horizontal border and the three below it
        const int b = (int)(t / J.nx), x = (int)(t - (long long)b * J.nx), y = (b + 1) * SGS_REG_TILE - 1;
        const unsigned a = (unsigned)y * (unsigned)J.nx + (unsigned)x;
        if (reg_load(&parent[a]) == SGS_REG_NONE) return;
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx != 0 && J.conn == 4) continue;
            const int xx = x + dx;
            if (xx < 0 || xx >= J.nx) continue;
            const unsigned o = a + (unsigned)J.nx + (unsigned)dx;
            if (reg_load(&parent[o]) != SGS_REG_NONE) reg_unite(parent, a, o, J.cells);
        }
        return;
    }
    t -= n_h;
    if (t < n_v) {
        // the cell left of a vertical border and the three right of it; a diagonal pair that also crosses a horizontal border belongs to the pass above
        const int b = (int)(t / J.ny), y = (int)(t - (long long)b * J.ny), x = (b + 1) * SGS_REG_TILE - 1;
        const unsigned a = (unsigned)y * (unsigned)J.nx + (unsigned)x;
        if (reg_load(&parent[a]) == SGS_REG_NONE) return;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (dy != 0 && (J.conn == 4 || yy < 0 || yy >= J.ny || yy / SGS_REG_TILE != y / SGS_REG_TILE)) continue;
            const unsigned o = (unsigned)yy * (unsigned)J.nx + (unsigned)x + 1u;
            if (reg_load(&parent[o]) != SGS_REG_NONE) reg_unite(parent, a, o, J.cells);
        }
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_flatten(RegionsJob J) {
    __shared__ unsigned s_cnt[2];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long m = blockIdx.y;
    const unsigned* parent = J.parent + m * (long long)J.cells;
    unsigned* root = J.root + m * (long long)J.cells;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    unsigned n_roots = 0, n_set = 0;
    for (int k = 0; k < SGS_REG_PER_THREAD; ++k) {
        const unsigned c = blockIdx.x * (unsigned)SGS_REG_CHUNK + (unsigned)(k * SGS_REG_THREADS + tid);
        unsigned r = SGS_REG_NONE;
        if (c < J.cells) {
            r = parent[c];
            if (r != SGS_REG_NONE)
                for (unsigned step = 0; step < J.cells; ++step) {
                    const unsigned p = parent[r];
                    if (p == r) break;
                    r = p;
                }
            root[c] = r;
        }
        n_roots += (unsigned)__popcll(__ballot(r == c && c < J.cells));
        n_set += (unsigned)__popcll(__ballot(r != SGS_REG_NONE));
    }
    if (lane == 0) {
        if (n_roots) atomicAdd(&s_cnt[0], n_roots);
        if (n_set) atomicAdd(&s_cnt[1], n_set);
    }
    __syncthreads();
    if (tid < 2) J.chunks[2 * (m * J.n_chunks + blockIdx.x) + tid] = s_cnt[tid];
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_scan(RegionsJob J) {
    __shared__ unsigned s_roots[SGS_REG_THREADS], s_set[SGS_REG_THREADS];
    const int tid = (int)threadIdx.x;
    const long long m = blockIdx.x;
    unsigned* chunks = J.chunks + 2 * m * J.n_chunks;
    const int per = (J.n_chunks + SGS_REG_THREADS - 1) / SGS_REG_THREADS;          // consecutive chunks of this thread
    const int c0 = min(tid * per, J.n_chunks), c1 = min(c0 + per, J.n_chunks);
    unsigned roots = 0, in_set = 0;
    for (int c = c0; c < c1; ++c) { roots += chunks[2 * c]; in_set += chunks[2 * c + 1]; }
    s_roots[tid] = roots; s_set[tid] = in_set;
    __syncthreads();
    unsigned base = 0;
    for (int u = 0; u < tid; ++u) base += s_roots[u];
    for (int c = c0; c < c1; ++c) { const unsigned n = chunks[2 * c]; chunks[2 * c] = base; base += n; }
    if (tid == SGS_REG_THREADS - 1) {
        unsigned total = 0;
        for (int u = 0; u < SGS_REG_THREADS; ++u) total += s_set[u];
        J.counts[4 * m] = base;
        J.counts[4 * m + 1] = total;
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_rank(RegionsJob J) {
    __shared__ unsigned s_n[SGS_REG_PER_THREAD * SGS_REG_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long m = blockIdx.y;
    unsigned* parent = J.parent + m * (long long)J.cells;
    const unsigned* root = J.root + m * (long long)J.cells;
    unsigned long long mine[SGS_REG_PER_THREAD];
    for (int k = 0; k < SGS_REG_PER_THREAD; ++k) {
        const unsigned c = blockIdx.x * (unsigned)SGS_REG_CHUNK + (unsigned)(k * SGS_REG_THREADS + tid);
        mine[k] = __ballot(c < J.cells && root[c] == c);
        if (lane == 0) s_n[k * SGS_REG_WAVES + wave] = (unsigned)__popcll(mine[k]);      // cell order in the chunk: k, then wave, then lane
    }
    __syncthreads();
    const unsigned base = J.chunks[2 * (m * J.n_chunks + blockIdx.x)];
    for (int k = 0; k < SGS_REG_PER_THREAD; ++k) {
        if (!((mine[k] >> lane) & 1ull)) continue;
        unsigned before = (unsigned)__popcll(mine[k] & ((1ull << lane) - 1ull));
        for (int u = 0; u < k * SGS_REG_WAVES + wave; ++u) before += s_n[u];
        const unsigned c = blockIdx.x * (unsigned)SGS_REG_CHUNK + (unsigned)(k * SGS_REG_THREADS + tid);
        parent[c] = base + before + 1u;
    }
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_labels(RegionsJob J) {
    const long long m = blockIdx.y;
    const unsigned* parent = J.parent + m * (long long)J.cells;
    unsigned* root = J.root + m * (long long)J.cells;
    int* labels = J.labels + m * (long long)J.cells;
    for (int k = 0; k < SGS_REG_PER_THREAD; ++k) {
        const unsigned c = blockIdx.x * (unsigned)SGS_REG_CHUNK + (unsigned)(k * SGS_REG_THREADS) + threadIdx.x;
        if (c >= J.cells) continue;
        const unsigned r = root[c];
        labels[c] = r == SGS_REG_NONE ? 0 : (int)parent[r];
        root[c] = 0;                                                               // area[c] from here on; nobody else reads root[c] in this launch
    }
}

__device__ __forceinline__ unsigned reg_slot(unsigned label) { return (label * SGS_REG_HASH) >> (32 - SGS_REG_SLOT_BITS); }

// One contribution of `n` cells of `label` (a run that has no slot, or a slot's total): the area of every label, the row of the labels that have one.
__device__ __forceinline__ void reg_send(const RegionsJob& J, long long m, unsigned label, unsigned n, unsigned x0, unsigned y0, unsigned x1, unsigned y1,
                                         unsigned first, unsigned long long sx, unsigned long long sy) {
    atomicAdd(&J.root[m * (long long)J.cells + (label - 1u)], n);
    if (label > (unsigned)J.max_regions) return;
    RegRow* r = &J.rows[m * (long long)J.max_regions + (label - 1u)];
    atomicAdd(&r->area, n);
    atomicMin(&r->x_min, x0);
    atomicMin(&r->y_min, y0);
    atomicMax(&r->x_end, x1);
    atomicMax(&r->y_end, y1);
    atomicMin(&r->first, first);
    atomicAdd(&r->sum_x, sx);
    atomicAdd(&r->sum_y, sy);
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_rows(RegionsJob J) {
    __shared__ unsigned s_key[SGS_REG_SLOTS], s_n[SGS_REG_SLOTS], s_x0[SGS_REG_SLOTS], s_y0[SGS_REG_SLOTS], s_x1[SGS_REG_SLOTS],
        s_y1[SGS_REG_SLOTS], s_first[SGS_REG_SLOTS];
    __shared__ unsigned long long s_sx[SGS_REG_SLOTS], s_sy[SGS_REG_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long m = blockIdx.y;
    const unsigned W = (unsigned)J.nx, HW = J.cells;
    const int* labels = J.labels + m * (long long)J.cells;
    for (int s = tid; s < SGS_REG_SLOTS; s += SGS_REG_THREADS) {
        s_key[s] = 0; s_n[s] = 0; s_x0[s] = 0x7FFFFFFFu; s_y0[s] = 0x7FFFFFFFu; s_x1[s] = 0; s_y1[s] = 0; s_first[s] = SGS_REG_NONE;
        s_sx[s] = 0; s_sy[s] = 0;
    }
    __syncthreads();
    // cell k of this thread is p0 + k * THREADS: the lanes of a wave hold 64 consecutive cells at every k
    const unsigned p0 = blockIdx.x * (unsigned)SGS_REG_ROW_REGION + (unsigned)tid;
    unsigned id[SGS_REG_ROW_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SGS_REG_ROW_PER_THREAD; ++k) {
        const unsigned p = p0 + (unsigned)k * SGS_REG_THREADS;
        id[k] = p < HW ? (unsigned)labels[p] : 0u;
    }
    // 1. every label of these cells proposes itself for its slot (one lane per change of label covers every label a wave holds)
#pragma unroll
    for (int k = 0; k < SGS_REG_ROW_PER_THREAD; ++k) {
        const unsigned v = id[k];
        const unsigned prev = __shfl_up(v, 1);
        if (v != 0 && (lane == 0 || v != prev)) atomicMax(&s_key[reg_slot(v)], v);
    }
    __syncthreads();
    // 2. runs: lanes next to each other on one row of the map with one label; the head lane contributes the run in closed form
    const unsigned step_y = SGS_REG_THREADS / W, step_x = SGS_REG_THREADS % W;
    unsigned y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int k = 0; k < SGS_REG_ROW_PER_THREAD; ++k) {
        const unsigned v = id[k];
        const bool in_label = v != 0;
        const unsigned prev = __shfl_up(v, 1);
        const bool head = in_label && (lane == 0 || x == 0 || v != prev);
        const unsigned long long starts = __ballot(!in_label || head);            // where a segment begins (bit 0 is always set)
        const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
        const int next = above ? lane + __ffsll((long long)above) : 64;           // the lane that begins the next segment
        if (head) {
            const unsigned len = (unsigned)(next - lane), first = p0 + (unsigned)k * SGS_REG_THREADS;
            const unsigned long long L = len;
            const unsigned long long sx = L * x + L * (L - 1) / 2, sy = L * y;
            const unsigned s = reg_slot(v);
            if (s_key[s] == v) {
                atomicAdd(&s_n[s], len);
                atomicMin(&s_x0[s], x);
                atomicMin(&s_y0[s], y);
                atomicMax(&s_x1[s], x + len);
                atomicMax(&s_y1[s], y + 1u);
                atomicMin(&s_first[s], first);
                atomicAdd(&s_sx[s], sx);
                atomicAdd(&s_sy[s], sy);
            }
            else reg_send(J, m, v, len, x, y, x + len, y + 1u, first, sx, sy);
        }
        x += step_x; y += step_y;
        if (x >= W) { x -= W; y += 1u; }
    }
    __syncthreads();
    // 3. one set of global atomics per label that owned a slot
    for (int s = tid; s < SGS_REG_SLOTS; s += SGS_REG_THREADS)
        if (s_key[s] != 0 && s_n[s] != 0) reg_send(J, m, s_key[s], s_n[s], s_x0[s], s_y0[s], s_x1[s], s_y1[s], s_first[s], s_sx[s], s_sy[s]);
}

__global__ __launch_bounds__(SGS_REG_THREADS) void k_reg_largest(RegionsJob J) {
    __shared__ unsigned s_area[SGS_REG_THREADS], s_label[SGS_REG_THREADS];
    const int tid = (int)threadIdx.x;
    const long long m = blockIdx.x;
    const unsigned* area = J.root + m * (long long)J.cells;
    const unsigned n = J.counts[4 * m];
    unsigned best = 0, label = 0;
    for (unsigned r = (unsigned)tid; r < n; r += SGS_REG_THREADS)                  // ascending labels: a tie keeps the smaller one
        if (area[r] > best) { best = area[r]; label = r + 1u; }
    s_area[tid] = best; s_label[tid] = label;
    __syncthreads();
    if (tid == 0) {
        for (int u = 1; u < SGS_REG_THREADS; ++u)
            if (s_area[u] > best || (s_area[u] == best && s_label[u] < label)) { best = s_area[u]; label = s_label[u]; }
        J.counts[4 * m + 2] = best;
        J.counts[4 * m + 3] = label;
    }
}

}  // namespace sgs
