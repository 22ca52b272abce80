// sgs_objects.h — gfx950 kernels of the per-frame visible-object table (sgs_object_table, include/sage_gs.h).
//
// From an id frame (int32 per pixel, as sgs_render_mesh_ids* writes it) and, optionally, the depth beside it: per frame one row per
// label — pixel count, tight box, sums of x and y, least depth — and two counters (pixels that show nothing, pixels whose id is no
// label).  THIS PROJECT'S OWN definition, like the id channel itself: the reference reads no such observation.
//
// Two stream-ordered launches:
//   k_obj_clear    writes the empty row into every row of every frame and zeroes the counters (what the output held does not matter)
//   k_obj_reduce   blockIdx.y = frame, blockIdx.x = a region of SGS_OBJ_REGION consecutive pixels of that frame (row-major, so a region
//                  is some whole image rows and two partial ones); a region never spans two frames
//
// Every field is an integer count, sum, minimum or maximum of non-negative values, so every contribution commutes: a frame's table
// depends on its pixels and n_labels alone, not on how the frame is cut into regions, waves and runs.  The reduction has three levels:
//   lanes      a wave holds 64 consecutive pixels.  Id frames are piecewise constant: lanes next to each other on one image row with one
//              label form a RUN.  A ballot of "in no label / differs from the previous lane / starts an image row" marks where segments
//              begin; the run's head lane contributes the whole run in closed form (length, first x, x + length, sum of x =
//              len x + len (len - 1) / 2, y len), and the depths of a run are folded by a segmented shuffle scan whose result the run's
//              last lane contributes.  A run never continues across the end of an image row.
//   LDS        a table of SGS_OBJ_SLOTS slots per workgroup, slot = obj_slot(label).  Ownership needs no compare-and-swap: every run
//              head of the region first proposes atomicMax(&key[slot], label + 1); after a barrier the key is final, and the runs whose
//              label owns its slot accumulate there with LDS atomics.  Runs whose label lost its slot (more labels in the region than
//              slots, or labels that collide) go straight to the global row — the same sums, minima and maxima, so the result is the same.
//   global     after a barrier, one set of integer atomics per (workgroup, label that owned a slot), and one add per counter.
// A whole-frame wall (one label, two million pixels) therefore costs one LDS update per wave and image row, and eight global atomics
// per region, not one per pixel.
//
// z_min is a minimum over the fp32 BIT PATTERNS read as uint32, starting from +inf (0x7F800000).  Negative numbers, -0 and NaNs of
// either sign have patterns above 0x7F800000 (the sign bit, or an all-ones exponent with a mantissa), so the unsigned minimum is the
// filter: they never enter, and +0, denormals, positive finite values and +inf do.  For the mesh path's frames that is the plain minimum.
//
// The atomics used are the ones every build has: atomicAdd (32- and 64-bit) and unsigned atomicMin / atomicMax.  x_min / y_min start
// at INT32_MAX and x_end / y_end at 0, and all values are non-negative, so the unsigned forms are exact on the row's int32 fields.
#pragma once
#include "sgs_common.h"

#define SGS_OBJ_THREADS 256
#define SGS_OBJ_PER_THREAD 8
#define SGS_OBJ_REGION (SGS_OBJ_THREADS * SGS_OBJ_PER_THREAD)      // pixels of a frame per workgroup
#define SGS_OBJ_SLOT_BITS 7
#define SGS_OBJ_SLOTS (1 << SGS_OBJ_SLOT_BITS)                     // rows of the workgroup's LDS table (44 bytes each)
#define SGS_OBJ_HASH 0x9E3779B1u                                   // slot = (label * SGS_OBJ_HASH) >> (32 - SGS_OBJ_SLOT_BITS)
#define SGS_OBJ_Z_INF 0x7F800000u                                  // +inf: an empty row's z_min, and the largest pattern that enters
#define SGS_OBJ_ID_NONE (-1)                                       // SGS_ID_NONE
#define SGS_OBJ_MAX_FRAMES 65535                                   // frames per k_obj_reduce launch (gridDim.y); more are issued in chunks

namespace sgs {

// sgs_object_row (include/sage_gs.h) as the kernels update it: the int32 fields through their unsigned views.
struct ObjRow {
    unsigned n_pixels;
    unsigned x_min, y_min, x_end, y_end;
    unsigned z_min;                        // fp32 bits
    unsigned long long sum_x, sum_y;
};
static_assert(sizeof(ObjRow) == 40, "sgs_object_row is 40 bytes");

struct ObjJob {
    const int* ids;                        // n_frames frames, stride elements apart
    const float* depth;                    // the same layout, or nullptr
    ObjRow* rows;                          // [n_frames][n_labels]
    unsigned* counts;                      // [n_frames][2]: SGS_ID_NONE pixels, pixels whose id is no label
    long long stride;
    int W, H, n_labels, n_frames;
};

__device__ __forceinline__ unsigned obj_slot(unsigned label) { return (label * SGS_OBJ_HASH) >> (32 - SGS_OBJ_SLOT_BITS); }

// One contribution to a global row (a run that has no slot, or a slot's total).  z goes by obj_send_z.
__device__ __forceinline__ void obj_send(ObjRow* r, unsigned n, unsigned x0, unsigned y0, unsigned x1, unsigned y1,
                                         unsigned long long sx, unsigned long long sy) {
    atomicAdd(&r->n_pixels, n);
    atomicMin(&r->x_min, x0);
    atomicMin(&r->y_min, y0);
    atomicMax(&r->x_end, x1);
    atomicMax(&r->y_end, y1);
    atomicAdd(&r->sum_x, sx);
    atomicAdd(&r->sum_y, sy);
}

__device__ __forceinline__ void obj_send_z(ObjRow* r, unsigned z) {
    if (z < SGS_OBJ_Z_INF) atomicMin(&r->z_min, z);
}

// Every row of every frame becomes the empty row; the counters become 0.
__global__ __launch_bounds__(SGS_OBJ_THREADS) void k_obj_clear(ObjJob J) {
    const long long n_rows = (long long)J.n_frames * J.n_labels, step = (long long)gridDim.x * SGS_OBJ_THREADS;
    const long long first = (long long)blockIdx.x * SGS_OBJ_THREADS + threadIdx.x;
    for (long long i = first; i < n_rows; i += step) {
        ObjRow e;
        e.n_pixels = 0; e.x_min = 0x7FFFFFFFu; e.y_min = 0x7FFFFFFFu; e.x_end = 0; e.y_end = 0; e.z_min = SGS_OBJ_Z_INF; e.sum_x = 0; e.sum_y = 0;
        J.rows[i] = e;
    }
    for (long long i = first; i < 2ll * J.n_frames; i += step) J.counts[i] = 0;
}

__global__ __launch_bounds__(SGS_OBJ_THREADS) void k_obj_reduce(ObjJob J) {
    __shared__ unsigned s_key[SGS_OBJ_SLOTS], s_n[SGS_OBJ_SLOTS], s_x0[SGS_OBJ_SLOTS], s_y0[SGS_OBJ_SLOTS], s_x1[SGS_OBJ_SLOTS],
        s_y1[SGS_OBJ_SLOTS], s_z[SGS_OBJ_SLOTS], s_cnt[2];
    __shared__ unsigned long long s_sx[SGS_OBJ_SLOTS], s_sy[SGS_OBJ_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const long long f = blockIdx.y;
    const unsigned W = (unsigned)J.W, HW = (unsigned)J.W * (unsigned)J.H;          // H W <= 2^31 - 1
    const int* ids = J.ids + f * J.stride;
    const float* depth = J.depth ? J.depth + f * J.stride : nullptr;
    ObjRow* rows = J.rows + f * J.n_labels;

    for (int s = tid; s < SGS_OBJ_SLOTS; s += SGS_OBJ_THREADS) {
        s_key[s] = 0; s_n[s] = 0; s_x0[s] = 0x7FFFFFFFu; s_y0[s] = 0x7FFFFFFFu; s_x1[s] = 0; s_y1[s] = 0; s_z[s] = SGS_OBJ_Z_INF;
        s_sx[s] = 0; s_sy[s] = 0;
    }
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();

    // pixel k of this thread is p0 + k * SGS_OBJ_THREADS (below 2^31 + SGS_OBJ_REGION: fits 32 bits): the lanes of a wave hold 64
    // consecutive pixels at every k
    const unsigned p0 = blockIdx.x * (unsigned)SGS_OBJ_REGION + (unsigned)tid;
    int id[SGS_OBJ_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SGS_OBJ_PER_THREAD; ++k) {
        const unsigned p = p0 + (unsigned)k * SGS_OBJ_THREADS;
        id[k] = p < HW ? ids[p] : SGS_OBJ_ID_NONE;
    }
    unsigned zb[SGS_OBJ_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SGS_OBJ_PER_THREAD; ++k) {
        const unsigned p = p0 + (unsigned)k * SGS_OBJ_THREADS;
        const bool in_label = p < HW && (unsigned)id[k] < (unsigned)J.n_labels;
        zb[k] = depth && in_label ? __float_as_uint(depth[p]) : SGS_OBJ_Z_INF;
    }

    // 1. every label of the region proposes itself for its slot (one lane per change of label is enough: it covers every label a wave holds)
#pragma unroll
    for (int k = 0; k < SGS_OBJ_PER_THREAD; ++k) {
        const int v = id[k];
        const int prev = __shfl_up(v, 1);
        if ((unsigned)v < (unsigned)J.n_labels && p0 + (unsigned)k * SGS_OBJ_THREADS < HW && (lane == 0 || v != prev))
            atomicMax(&s_key[obj_slot((unsigned)v)], (unsigned)v + 1u);
    }
    __syncthreads();

    // 2. runs
    const unsigned step_y = SGS_OBJ_THREADS / W, step_x = SGS_OBJ_THREADS % W;
    unsigned y = p0 / W, x = p0 - y * W;
    unsigned n_none = 0, n_other = 0;
#pragma unroll
    for (int k = 0; k < SGS_OBJ_PER_THREAD; ++k) {
        const int v = id[k];
        const bool valid = p0 + (unsigned)k * SGS_OBJ_THREADS < HW;
        const bool in_label = valid && (unsigned)v < (unsigned)J.n_labels;
        const int prev = __shfl_up(v, 1);
        const bool head = in_label && (lane == 0 || x == 0 || v != prev);
        const unsigned long long starts = __ballot(!in_label || head);            // where a segment begins (bit 0 is always set)
        n_none += (unsigned)__popcll(__ballot(valid && v == SGS_OBJ_ID_NONE));
        n_other += (unsigned)__popcll(__ballot(valid && !in_label && v != SGS_OBJ_ID_NONE));
        const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
        const int next = above ? lane + __ffsll((long long)above) : 64;           // the lane that begins the next segment
        const bool own = in_label && s_key[obj_slot((unsigned)v)] == (unsigned)v + 1u;
        if (head) {
            const unsigned len = (unsigned)(next - lane);
            const unsigned long long L = len;
            const unsigned long long sx = L * x + L * (L - 1) / 2, sy = L * y;
            if (own) {
                const unsigned s = obj_slot((unsigned)v);
                atomicAdd(&s_n[s], len);
                atomicMin(&s_x0[s], x);
                atomicMin(&s_y0[s], y);
                atomicMax(&s_x1[s], x + len);
                atomicMax(&s_y1[s], y + 1u);
                atomicAdd(&s_sx[s], sx);
                atomicAdd(&s_sy[s], sy);
            }
            else obj_send(&rows[v], len, x, y, x + len, y + 1u, sx, sy);
        }
        if (depth) {                                                             // (uniform)
            // segmented minimum scan: after it the last lane of a run holds the least pattern of the run
            const int seg = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
            unsigned z = zb[k];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(z, d);
                if (lane - d >= seg) z = min(z, o);
            }
            if (in_label && next == lane + 1 && z < SGS_OBJ_Z_INF) {
                if (own) atomicMin(&s_z[obj_slot((unsigned)v)], z);
                else obj_send_z(&rows[v], z);
            }
        }
        x += step_x; y += step_y;
        if (x >= W) { x -= W; y += 1u; }
    }
    if (lane == 0) {
        if (n_none) atomicAdd(&s_cnt[0], n_none);
        if (n_other) atomicAdd(&s_cnt[1], n_other);
    }
    __syncthreads();

    // 3. one set of global atomics per label that owned a slot
    for (int s = tid; s < SGS_OBJ_SLOTS; s += SGS_OBJ_THREADS) {
        if (s_key[s] == 0 || s_n[s] == 0) continue;
        ObjRow* r = &rows[s_key[s] - 1u];
        obj_send(r, s_n[s], s_x0[s], s_y0[s], s_x1[s], s_y1[s], s_sx[s], s_sy[s]);
        obj_send_z(r, s_z[s]);
    }
    if (tid < 2 && s_cnt[tid]) atomicAdd(&J.counts[2 * f + tid], s_cnt[tid]);
}

}  // namespace sgs
