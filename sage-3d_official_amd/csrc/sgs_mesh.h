// sgs_mesh.h — gfx950 kernels of the collision-mesh depth and object-id path (sgs_render_mesh_depth*, sgs_render_mesh_ids*,
// include/sage_gs.h).
//
// A group of up to SGS_MESH_MAX_GROUP frames of one resolution is five stream-ordered launches with no host synchronisation in between:
//   k_mesh_setup      one thread per (triangle, frame): fp64 transform, cull, 16-float record, tile rect of the part with z >= near_z
//   k_mesh_bin<0>     per-tile counts: a rect of at most SGS_MESH_SMALL tiles is walked by its own thread, a larger one by a wave
//   k_mesh_scan       one workgroup per frame: exclusive scan of the counts -> tile offsets, D, the longest list
//   k_mesh_bin<1>     the same walk again, scattering triangle ids into the per-tile lists (the record buffer)
//   k_mesh_depth      one 256-lane workgroup per 16x16-pixel tile: the list's records staged through LDS, a running min per pixel
//   (k_mesh_ids       in its place for sgs_render_mesh_ids*: the same walk, a running min of (z, label) per pixel)
// The result of a pixel is a MINIMUM over the triangles its tile lists, so it depends neither on the order of a list nor on which other
// tiles / frames share the launches: batch, band and single frame agree bit for bit, as do permutations of the triangles.
//
// Watertightness: the inside test of pixel ray r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) against triangle (p0, p1, p2) is
// sign(det) * e_k . r >= 0 for the three edge planes e_k = p_a x p_b through the camera (homogeneous edge functions in camera space: no
// projection, no division, linear in r; the mirrored cone behind the camera is what the z > near_z test removes).  Two triangles that
// share an edge compute its e from the same two fp64 vertices, in the order of their indices (lower first) and with a product that is
// anti-commutative bit for bit (mul and sub each rounded on their own, never fused), then round it to fp32 and flip its sign exactly.
// Both then evaluate +-the same fp32 value at every pixel, and e . r == 0 counts as inside for both: no pixel falls between them.
// A vertex needs more: each edge plane through it is rounded to fp32 on its own, so the rounded planes no longer meet in one line, and a
// ray within that rounding of the vertex can see every edge through it with one strict sign (no triangle of the fan would claim it).  So
// an edge whose fp32 value is negative but within the fp32 error bound of 0 (the record's prefilter w: 8 u max_k |e_k|_1, times
// max(1, |rx|, |ry|)) is decided again in fp64 (mesh_edge64): the same index-ordered plane, kept in fp64, passes when its value is
// >= -2^-50 sum_i P_i |r_i|, P the plane's products — above the fp64 rounding of the plane and of its evaluation.  Planes through one
// vertex meet in one line up to that rounding, so some triangle of every fan passes; the rule is +-symmetric across a shared edge too,
// and it only adds pixels within rounding of an edge (tests/mesh_depth_ref.py, "Edge-exact bounds").
#pragma once
#include "sgs_common.h"

#define SGS_MESH_MAX_GROUP 8        // frames per set of launches (blockIdx.y = frame)
#define SGS_MESH_SMALL 16           // rects of at most this many tiles are binned by one thread; larger ones by a whole wave
#define SGS_MESH_BIN_BLOCKS 1024    // binning workgroups (grid-stride over the triangles)
#define SGS_MESH_SCAN_THREADS 1024

namespace sgs {

struct MeshFrame {
    float view[12];                 // model -> camera, rows of a rigid 3x4
    float fx, fy, cx, cy, near_z, far_z;
    int32_t width, height;
    int32_t gx;                     // tiles per row
    int32_t row_begin, row_end;     // the band of tile rows [row_begin, row_end) of the frame
    float* out;                     // the frame's H*W depth buffer (k_mesh_ids: nullable)
    int32_t* out_id;                // k_mesh_ids: the frame's H*W label buffer
};

struct MeshStatus {
    unsigned n_visible;             // triangles with a non-empty rect in the band
    unsigned d_total;               // records of the frame
    unsigned max_tile_len;
    unsigned n_big;                 // entries of the frame's big-rect list
};

struct MeshGroup {
    MeshFrame f[SGS_MESH_MAX_GROUP];
    int32_t nf;
    int32_t n_tiles;                // tiles of one frame's band (the same for every frame of the group)
    long long n_tris;
    long long cap;                  // entries the record buffer holds
    const float* verts;             // [V][3]
    const int* tris;                // [F][3]
    const int* labels;              // k_mesh_ids: [F] labels >= 0, or NULL: a triangle's label is its index
    float4* rec;                    // [nf][F][4]: (e0, 0) (e1, 0) (e2, 0) (n, n.p0), edges already multiplied by sign(det)
    uint2* rect;                    // [nf][F]: tile rect, x0 | x1 << 16, y0 | y1 << 16 (x0 > x1: empty)
    unsigned* big;                  // [nf][F]: triangles whose rect exceeds SGS_MESH_SMALL tiles
    unsigned* counts;               // [nf][n_tiles]: per-tile counts, then the emit's cursors (zeroed before every group)
    unsigned* offs;                 // [nf][n_tiles + 1]: offsets within the frame's part of the record buffer
    unsigned* list;                 // the record buffer: triangle ids, frame after frame
    MeshStatus* st;                 // [nf] (zeroed before every group)
};

// Upload check: every vertex finite (bit 0 of *bad), every index in [0, n_verts) (bit 1).
__global__ __launch_bounds__(256) void k_mesh_validate(long long n_verts, const float* __restrict__ verts, long long n_tris,
                                                      const int* __restrict__ tris, unsigned* __restrict__ bad) {
    unsigned flags = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n_verts; i += stride)
        if ((__float_as_uint(verts[i]) & 0x7f800000u) == 0x7f800000u) flags |= 1u;     // inf / NaN
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n_tris; i += stride)
        if (tris[i] < 0 || (long long)tris[i] >= n_verts) flags |= 2u;
    if (flags) atomicOr(bad, flags);
}

// sgs_mesh_set_labels' check: every label in [0, INT32_MAX - 1] (bit 2 of *bad).
__global__ __launch_bounds__(256) void k_mesh_validate_labels(long long n_tris, const int* __restrict__ labels, unsigned* __restrict__ bad) {
    unsigned flags = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_tris; i += stride)
        if (labels[i] < 0 || labels[i] == 0x7fffffff) flags |= 4u;
    if (flags) atomicOr(bad, flags);
}

struct MeshD3 { double x, y, z; };

// a x b with every product and difference rounded on its own: b x a == -(a x b) exactly
__device__ __forceinline__ MeshD3 mesh_cross_rn(const MeshD3& a, const MeshD3& b) {
    return MeshD3{__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
                  __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x))};
}

// Camera-space vertex in fp64 with explicit fmas: the same vertex gives the same bits in every triangle (and kernel) that uses it.
__device__ __forceinline__ MeshD3 mesh_vertex(const MeshFrame& F, const float* v) {
    const double x = v[0], y = v[1], z = v[2];
    return MeshD3{fma((double)F.view[0], x, fma((double)F.view[1], y, fma((double)F.view[2], z, (double)F.view[3]))),
                  fma((double)F.view[4], x, fma((double)F.view[5], y, fma((double)F.view[6], z, (double)F.view[7]))),
                  fma((double)F.view[8], x, fma((double)F.view[9], y, fma((double)F.view[10], z, (double)F.view[11])))};
}

__device__ __forceinline__ unsigned mesh_tile_of(int x, int y, const MeshFrame& F) { return (unsigned)((y - F.row_begin) * F.gx + x); }

__global__ __launch_bounds__(256) void k_mesh_setup(const MeshGroup G) {
    const int f = blockIdx.y;
    const MeshFrame& F = G.f[f];
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool live = false;
    if (t < G.n_tris) {
        const size_t slot = (size_t)f * (size_t)G.n_tris + (size_t)t;
        uint2 rect = make_uint2(1u, 1u);                    // empty
        int idx[3];
        MeshD3 p[3];
        for (int k = 0; k < 3; ++k) {
            idx[k] = G.tris[3 * t + k];
            p[k] = mesh_vertex(F, G.verts + 3 * (size_t)idx[k]);
        }
        const double nz = F.near_z, fz = F.far_z, W = F.width, H = F.height;
        const bool behind = p[0].z <= nz && p[1].z <= nz && p[2].z <= nz;
        const bool beyond = p[0].z > fz && p[1].z > fz && p[2].z > fz;
        // side planes of the whole frame (a band only clamps the rect, so that a band sees exactly the triangles the full frame does)
        bool out_l = true, out_r = true, out_t = true, out_b = true;
        for (int k = 0; k < 3; ++k) {
            out_l = out_l && (F.fx * p[k].x + F.cx * p[k].z < 0.0);
            out_r = out_r && (F.fx * p[k].x + (F.cx - W) * p[k].z > 0.0);
            out_t = out_t && (F.fy * p[k].y + F.cy * p[k].z < 0.0);
            out_b = out_b && (F.fy * p[k].y + (F.cy - H) * p[k].z > 0.0);
        }
        const MeshD3 c12 = mesh_cross_rn(p[1], p[2]);
        const double det = c12.x * p[0].x + c12.y * p[0].y + c12.z * p[0].z;
        if (!behind && !beyond && !out_l && !out_r && !out_t && !out_b && det != 0.0 && det == det) {
            // tile rect of the part with z >= near_z (a triangle that straddles the camera plane projects without bound otherwise)
            double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
            for (int k = 0; k < 3; ++k) {
                const MeshD3& a = p[k];
                const MeshD3& b = p[(k + 1) % 3];
                MeshD3 q[2];
                int nq = 0;
                if (a.z >= nz) q[nq++] = a;
                if ((a.z >= nz) != (b.z >= nz)) {
                    const double s = (nz - a.z) / (b.z - a.z);
                    q[nq++] = MeshD3{a.x + s * (b.x - a.x), a.y + s * (b.y - a.y), nz};
                }
                for (int j = 0; j < nq; ++j) {
                    const double iz = 1.0 / q[j].z;
                    const double u = fmin(fmax(F.fx * q[j].x * iz + F.cx, -2.0), W + 2.0);
                    const double v = fmin(fmax(F.fy * q[j].y * iz + F.cy, -2.0), H + 2.0);
                    umin = fmin(umin, u); umax = fmax(umax, u); vmin = fmin(vmin, v); vmax = fmax(vmax, v);
                }
            }
            if (umin <= umax) {
                // pixel x is sampled at u = x + 0.5; one pixel of slack on each side for the fp32 edge tests
                const int x0 = max((int)floor(umin) - 1, 0), x1 = min((int)floor(umax) + 1, F.width - 1);
                const int y0 = max((int)floor(vmin) - 1, 0), y1 = min((int)floor(vmax) + 1, F.height - 1);
                const int tx0 = x0 >> 4, tx1 = x1 >> 4;
                const int ty0 = max(y0 >> 4, F.row_begin), ty1 = min(y1 >> 4, F.row_end - 1);
                if (x0 <= x1 && ty0 <= ty1) {
                    live = true;
                    rect = make_uint2((unsigned)tx0 | ((unsigned)tx1 << 16), (unsigned)ty0 | ((unsigned)ty1 << 16));
                    const double sg = det > 0.0 ? 1.0 : -1.0;
                    float4* R = G.rec + 4 * slot;
                    double l1 = 0.0;
                    for (int k = 0; k < 3; ++k) {
                        const int a = (k + 1) % 3, b = (k + 2) % 3;
                        // the edge's plane from its vertices in index order, sign flipped exactly afterwards
                        const bool swap = idx[a] > idx[b];
                        const MeshD3 e = swap ? mesh_cross_rn(p[b], p[a]) : mesh_cross_rn(p[a], p[b]);
                        const double s = swap ? -sg : sg;
                        R[k] = make_float4((float)(s * e.x), (float)(s * e.y), (float)(s * e.z), 0.f);
                        l1 = fmax(l1, fabs(e.x) + fabs(e.y) + fabs(e.z));
                    }
                    R[0].w = (float)(0x1p-21 * l1);         // the fp64 recheck's prefilter: 8 u max_k |e_k|_1

                    const MeshD3 u1{p[1].x - p[0].x, p[1].y - p[0].y, p[1].z - p[0].z}, u2{p[2].x - p[0].x, p[2].y - p[0].y, p[2].z - p[0].z};
                    const MeshD3 n{u1.y * u2.z - u1.z * u2.y, u1.z * u2.x - u1.x * u2.z, u1.x * u2.y - u1.y * u2.x};
                    R[3] = make_float4((float)n.x, (float)n.y, (float)n.z, (float)(n.x * p[0].x + n.y * p[0].y + n.z * p[0].z));
                    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > SGS_MESH_SMALL) {
                        const unsigned k = atomicAdd(&G.st[f].n_big, 1u);
                        G.big[(size_t)f * (size_t)G.n_tris + k] = (unsigned)t;
                    }
                }
            }
        }
        G.rect[slot] = rect;
    }
    const unsigned long long m = __ballot(live);
    if ((threadIdx.x & (SGS_WAVE - 1)) == 0 && m) atomicAdd(&G.st[f].n_visible, (unsigned)__popcll(m));
}

// The frame's base in the record buffer: the records of the frames before it in the group.
__device__ __forceinline__ unsigned long long mesh_base(const MeshGroup& G, int f) {
    unsigned long long b = 0;
    for (int g = 0; g < f; ++g) b += G.st[g].d_total;
    return b;
}

template <bool EMIT>
__device__ __forceinline__ void mesh_bin_one(const MeshGroup& G, int f, unsigned tile, unsigned tri, unsigned long long base) {
    unsigned* c = G.counts + (size_t)f * G.n_tiles + tile;
    if (!EMIT) {
        atomicAdd(c, 1u);
    } else {
        const unsigned long long pos = base + G.offs[(size_t)f * (G.n_tiles + 1) + tile] + atomicAdd(c, 1u);
        if (pos < (unsigned long long)G.cap) G.list[pos] = tri;
    }
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_mesh_bin(const MeshGroup G) {
    const int f = blockIdx.y;
    const MeshFrame& F = G.f[f];
    const unsigned long long base = EMIT ? mesh_base(G, f) : 0ull;
    const uint2* rects = G.rect + (size_t)f * (size_t)G.n_tris;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < G.n_tris; t += (long long)gridDim.x * blockDim.x) {
        const uint2 r = rects[t];
        const int x0 = r.x & 0xffff, x1 = r.x >> 16, y0 = r.y & 0xffff, y1 = r.y >> 16;
        if (x0 > x1 || y0 > y1 || (x1 - x0 + 1) * (y1 - y0 + 1) > SGS_MESH_SMALL) continue;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) mesh_bin_one<EMIT>(G, f, mesh_tile_of(x, y, F), (unsigned)t, base);
    }
    // large rects (walls, floors): a wave per triangle, a lane per tile
    const unsigned n_big = G.st[f].n_big;
    const unsigned lane = threadIdx.x & (SGS_WAVE - 1);
    const unsigned waves = blockDim.x / SGS_WAVE;
    for (unsigned k = blockIdx.x * waves + threadIdx.x / SGS_WAVE; k < n_big; k += gridDim.x * waves) {
        const unsigned t = G.big[(size_t)f * (size_t)G.n_tris + k];
        const uint2 r = rects[t];
        const int x0 = r.x & 0xffff, x1 = r.x >> 16, y0 = r.y & 0xffff, y1 = r.y >> 16;
        const int w = x1 - x0 + 1, area = w * (y1 - y0 + 1);
        for (int j = (int)lane; j < area; j += SGS_WAVE) mesh_bin_one<EMIT>(G, f, mesh_tile_of(x0 + j % w, y0 + j / w, F), t, base);
    }
}

// One workgroup per frame: offs = exclusive scan of counts, counts zeroed (they are the emit's cursors next).
__global__ __launch_bounds__(SGS_MESH_SCAN_THREADS) void k_mesh_scan(const MeshGroup G) {
    __shared__ unsigned s_wave[SGS_MESH_SCAN_THREADS / SGS_WAVE];
    __shared__ unsigned s_carry, s_max;
    const int f = blockIdx.y;
    const unsigned tid = threadIdx.x, lane = tid & (SGS_WAVE - 1), wv = tid / SGS_WAVE;
    unsigned* counts = G.counts + (size_t)f * G.n_tiles;
    unsigned* offs = G.offs + (size_t)f * (G.n_tiles + 1);
    if (tid == 0) { s_carry = 0; s_max = 0; }
    __syncthreads();
    for (int b = 0; b < G.n_tiles; b += SGS_MESH_SCAN_THREADS) {
        const int i = b + (int)tid;
        const unsigned v = i < G.n_tiles ? counts[i] : 0u;
        unsigned inc = v;
        for (int d = 1; d < SGS_WAVE; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if ((int)lane >= d) inc += o;
        }
        if (lane == SGS_WAVE - 1) s_wave[wv] = inc;
        if (v) atomicMax(&s_max, v);
        __syncthreads();
        if (wv == 0) {
            const unsigned w = lane < SGS_MESH_SCAN_THREADS / SGS_WAVE ? s_wave[lane] : 0u;
            unsigned winc = w;
            for (int d = 1; d < SGS_MESH_SCAN_THREADS / SGS_WAVE; d <<= 1) {
                const unsigned o = __shfl_up(winc, d);
                if ((int)lane >= d) winc += o;
            }
            if (lane < SGS_MESH_SCAN_THREADS / SGS_WAVE) s_wave[lane] = winc - w;       // exclusive prefix of the waves
        }
        __syncthreads();
        const unsigned carry = s_carry;
        if (i < G.n_tiles) { offs[i] = carry + s_wave[wv] + inc - v; counts[i] = 0u; }
        __syncthreads();
        if (tid == SGS_MESH_SCAN_THREADS - 1) s_carry = carry + s_wave[wv] + inc;
        __syncthreads();
    }
    if (tid == 0) {
        offs[G.n_tiles] = s_carry;
        G.st[f].d_total = s_carry;
        G.st[f].max_tile_len = s_max;
    }
}

// The inside test of triangle t at ray (rx, ry, 1) when its fp32 edge values s[] are not all >= 0 but within rounding of 0 (header):
// every edge with s < 0 is decided again from its fp64 plane, built exactly as k_mesh_setup builds it before rounding.
__device__ __forceinline__ bool mesh_inside64(const MeshGroup& G, const MeshFrame& F, unsigned t, const float4* e32, const float* s, float rx,
                                           float ry) {
    int idx[3];
    MeshD3 p[3];
    for (int k = 0; k < 3; ++k) {
        idx[k] = G.tris[3 * (size_t)t + k];
        p[k] = mesh_vertex(F, G.verts + 3 * (size_t)idx[k]);
    }
    const double x = rx, y = ry, ax = fabs(x), ay = fabs(y);
    for (int k = 0; k < 3; ++k) {
        if (s[k] >= 0.f) continue;
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const bool swap = idx[a] > idx[b];
        const MeshD3& u = swap ? p[b] : p[a];
        const MeshD3& v = swap ? p[a] : p[b];
        const MeshD3 e = mesh_cross_rn(u, v);
        // the record holds this plane times +-1, rounded: its sign is the sign of their dot product
        const double sg = (double)e32[k].x * e.x + (double)e32[k].y * e.y + (double)e32[k].z * e.z >= 0.0 ? 1.0 : -1.0;
        const double g = fma(sg * e.x, x, fma(sg * e.y, y, sg * e.z));
        const double Px = fabs(u.y * v.z) + fabs(u.z * v.y), Py = fabs(u.z * v.x) + fabs(u.x * v.z), Pz = fabs(u.x * v.y) + fabs(u.y * v.x);
        if (!(g >= -0x1p-50 * fma(Px, ax, fma(Py, ay, Pz)))) return false;
    }
    return true;
}

// The per-record test both last-stage kernels share, so that they can never disagree about a hit: record k of the staged batch against
// the lane's ray — the fp32 edge functions, the fp64 re-decision of an edge within rounding of 0, z and the near / far rule.  Returns the
// hit's z, or +inf when the ray misses the triangle or z is outside (near_z, far_z].
__device__ __forceinline__ float mesh_hit(const MeshGroup& G, const MeshFrame& F, const float4 (*s_rec)[256], const unsigned* s_id, int k, float rx,
                                          float ry, float rmax, float near_z, float far_z) {
    float best = __uint_as_float(0x7f800000u);
    const float4 e0 = s_rec[0][k], e1 = s_rec[1][k], e2 = s_rec[2][k];
    const float s0 = fmaf(e0.x, rx, fmaf(e0.y, ry, e0.z));
    const float s1 = fmaf(e1.x, rx, fmaf(e1.y, ry, e1.z));
    const float s2 = fmaf(e2.x, rx, fmaf(e2.y, ry, e2.z));
    bool in = s0 >= 0.f && s1 >= 0.f && s2 >= 0.f;
    if (!in && fmaf(e0.w, rmax, fminf(s0, fminf(s1, s2))) >= 0.f) {         // within rounding of an edge: fp64 (header)
        const float4 e[3] = {e0, e1, e2};
        const float sv[3] = {s0, s1, s2};
        in = mesh_inside64(G, F, s_id[k], e, sv, rx, ry);
    }
    if (in) {
        const float4 pl = s_rec[3][k];
        const float z = pl.w / fmaf(pl.x, rx, fmaf(pl.y, ry, pl.z));
        if (z > near_z && z <= far_z) best = z;
    }
    return best;
}

// The last stage of a tile: one 256-lane workgroup, one pixel per lane, the tile's list staged through LDS 256 records at a time.
// IDS = false (k_mesh_depth): a running minimum of z per lane.  IDS = true (k_mesh_ids): each record's label is staged beside its id and
// the lane keeps the minimum of the PAIR (z, label) in that order — the least fp32 z, the least label among hits whose z is bit-equal —
// so the id belongs to the depth the same walk reports, and neither depends on the order of the list.  Two plain compares and a select
// per record, not a packed 64-bit key (the bits of a float order as its value only while it is positive): noise beside the three edge
// functions, in a kernel bound by its longest list walked serially.
template <bool IDS>
__device__ __forceinline__ void mesh_tile_walk(const MeshGroup& G) {
    __shared__ float4 s_rec[4][256];
    __shared__ unsigned s_id[256];
    __shared__ int s_label[IDS ? 256 : 1];
    const int f = blockIdx.y;
    const MeshFrame& F = G.f[f];
    unsigned long long total = 0, base = 0;
    for (int g = 0; g < G.nf; ++g) { if (g == f) base = total; total += G.st[g].d_total; }
    if (total > (unsigned long long)G.cap) return;           // overflow: the host grows the record buffer and renders again
    const unsigned tile = blockIdx.x;
    const unsigned* offs = G.offs + (size_t)f * (G.n_tiles + 1);
    const unsigned long long begin = base + offs[tile], end = base + offs[tile + 1];
    const int px = (int)(tile % (unsigned)F.gx) * SGS_TILE_PX + (int)(threadIdx.x & 15);
    const int py = (F.row_begin + (int)(tile / (unsigned)F.gx)) * SGS_TILE_PX + (int)(threadIdx.x >> 4);
    const float rx = ((float)px + 0.5f - F.cx) / F.fx, ry = ((float)py + 0.5f - F.cy) / F.fy;
    const float rmax = fmaxf(1.f, fmaxf(fabsf(rx), fabsf(ry)));
    const float near_z = F.near_z, far_z = F.far_z;
    const float4* rec = G.rec + 4 * (size_t)f * (size_t)G.n_tris;
    float best = __uint_as_float(0x7f800000u);
    int best_label = SGS_ID_NONE;                            // (a label is >= 0: a miss, z = +inf, never replaces it)
    for (unsigned long long b = begin; b < end; b += 256) {
        const int n = end - b < 256ull ? (int)(end - b) : 256;
        if ((int)threadIdx.x < n) {
            const unsigned id = G.list[b + threadIdx.x];
            const float4* R = rec + 4 * (size_t)id;
            s_id[threadIdx.x] = id;
            if (IDS) s_label[threadIdx.x] = G.labels ? G.labels[id] : (int)id;
            s_rec[0][threadIdx.x] = R[0]; s_rec[1][threadIdx.x] = R[1]; s_rec[2][threadIdx.x] = R[2]; s_rec[3][threadIdx.x] = R[3];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float z = mesh_hit(G, F, s_rec, s_id, k, rx, ry, rmax, near_z, far_z);
            if (IDS) {
                const int label = s_label[k];
                if (z < best || (z == best && label < best_label)) { best = z; best_label = label; }
            } else {
                best = fminf(best, z);
            }
        }
        __syncthreads();
    }
    if (px < F.width && py < F.height) {
        if (!IDS || F.out) F.out[(size_t)py * F.width + px] = best;
        if (IDS) F.out_id[(size_t)py * F.width + px] = best_label;
    }
}

__global__ __launch_bounds__(256) void k_mesh_depth(const MeshGroup G) { mesh_tile_walk<false>(G); }

// sgs_render_mesh_ids*: per pixel the label of the hit the depth frame reports (SGS_ID_NONE where nothing is hit), and that depth.
__global__ __launch_bounds__(256) void k_mesh_ids(const MeshGroup G) { mesh_tile_walk<true>(G); }

}  // namespace sgs
