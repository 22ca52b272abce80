// sgs_resize.h — gfx950 kernels of the frame resize (sgs_resize, include/sage_gs.h).
//
// Two filters on two kinds of frame.  Bicubic is Pillow's separable convolution resampling (Image.resize at its default resample),
// restated from its documented behaviour and pinned to its output bit for bit by the tests; linear is bilinear at half-pixel centres,
// defined exactly in include/sage_gs.h.  The reference resizes on the host (run_benchmark.py:1409-1419, 1441-1451; simple_env.py:2750).
//
// Bicubic is two stream-ordered launches through an intermediate in the library's scratch:
//   k_resize_h   one thread per pixel of the [H, w] intermediate (all three channels): takes the fp32 frame to levels as it loads (RGB8)
//                or clips it (F32), convolves along x, writes one packed RGBX word (RGB8: the 8-bit levels) or one fp32 (F32)
//   k_resize_v   one thread per pixel of dst: convolves the intermediate along y — one word per tap — and writes the frame
// A pass whose in-size equals its out-size is skipped (never run with identity weights): the remaining pass then reads the frame or
// writes dst itself; with both skipped k_resize_copy writes the quantised (clipped) frame.  Linear is one launch, k_resize_linear.
//
// The tap table of an axis (ResizeAxis: the window's first tap and length per output, then the weights — int32 of 22 fractional bits
// for RGB8, fp64 for F32) is computed on the host by resize::build_axis and kept by the context per (in-size, out-size, filter, format).
//
// Arithmetic that must not depend on the compiler is written unfused (#pragma clang fp contract(off): hipcc contracts by default, the
// host compiler of the CPU test build does not): the coefficients and the fp64 sums of the F32 path.  The RGB8 level is k_pack_rgba8's
// expression and is contracted or not exactly as it is there; everything after the levels is integer arithmetic.
#pragma once
#include <cmath>
#include <vector>

#include "sgs_common.h"

#define SGS_RESIZE_THREADS 256
#define SGS_RESIZE_BITS 22                 // fractional bits of an RGB8 weight

namespace sgs {

enum { RESIZE_RGB8 = 0, RESIZE_F32 = 1 };

struct ResizeAxis {
    const int* bounds;                     // [out][2]: first tap, taps
    const int* ki;                         // RGB8: [out][ksize] weights of SGS_RESIZE_BITS fractional bits
    const double* kd;                      // F32:  [out][ksize]
    int ksize;
};

struct ResizeJob {
    const float* src;                      // n_frames frames, src_stride floats apart
    float* dst;
    long long src_stride, dst_stride;
    int W, H, w, h;                        // in-size, out-size
    float clip_lo, clip_hi;
    unsigned* mid;                         // [n_frames][H][w]: RGBX levels (RGB8) or fp32 bits (F32); used when both passes run
    ResizeAxis ax, ay;
    int h_to_dst;                          // the vertical pass is skipped: k_resize_h writes dst
    int v_from_src;                        // the horizontal pass is skipped: k_resize_v reads src
};

// k_pack_rgba8's level of one channel.
__device__ __forceinline__ int resize_level(float x) {
    const float c = fminf(fmaxf(x, 0.f), 1.f);
    return (int)(unsigned)(c * 255.0f + 0.5f);
}

__device__ __forceinline__ float resize_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ unsigned resize_clamp8(int s) {
    const int v = s >> SGS_RESIZE_BITS;    // arithmetic shift
    return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// The fp32 nearest k / 255: one correctly rounded division.
__device__ __forceinline__ float resize_unlevel(unsigned k) { return (float)k / 255.0f; }

__device__ __forceinline__ void resize_store_rgb(float* p, unsigned r, unsigned g, unsigned b) {
    p[0] = resize_unlevel(r); p[1] = resize_unlevel(g); p[2] = resize_unlevel(b);
}

// Horizontal pass: [H, W] -> [H, w].
template <int FMT>
__global__ __launch_bounds__(SGS_RESIZE_THREADS) void k_resize_h(ResizeJob J) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const long long i = (long long)blockIdx.x * SGS_RESIZE_THREADS + threadIdx.x;
    if (i >= (long long)J.w * J.H) return;
    const int y = (int)(i / J.w), x = (int)(i - (long long)y * J.w);
    const long long f = blockIdx.y;
    const int lo = J.ax.bounds[2 * x], n = J.ax.bounds[2 * x + 1];
    if (FMT == RESIZE_RGB8) {
        const float* row = J.src + f * J.src_stride + ((long long)y * J.W + lo) * 3;
        const int* kk = J.ax.ki + (long long)x * J.ax.ksize;
        int r = 1 << (SGS_RESIZE_BITS - 1), g = r, b = r;
        for (int j = 0; j < n; ++j) {
            const int k = kk[j];
            r += resize_level(row[3 * j]) * k; g += resize_level(row[3 * j + 1]) * k; b += resize_level(row[3 * j + 2]) * k;
        }
        const unsigned R = resize_clamp8(r), G = resize_clamp8(g), B = resize_clamp8(b);
        if (J.h_to_dst) resize_store_rgb(J.dst + f * J.dst_stride + 3 * i, R, G, B);
        else J.mid[f * J.H * J.w + i] = R | (G << 8) | (B << 16);
    } else {
        const float* row = J.src + f * J.src_stride + (long long)y * J.W + lo;
        const double* kd = J.ax.kd + (long long)x * J.ax.ksize;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = s + (double)resize_clip(row[j], J.clip_lo, J.clip_hi) * kd[j];
        const float v = (float)s;
        if (J.h_to_dst) J.dst[f * J.dst_stride + i] = v;
        else J.mid[f * J.H * J.w + i] = __float_as_uint(v);
    }
}

// Vertical pass: [H, w] -> [h, w].
template <int FMT>
__global__ __launch_bounds__(SGS_RESIZE_THREADS) void k_resize_v(ResizeJob J) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const long long i = (long long)blockIdx.x * SGS_RESIZE_THREADS + threadIdx.x;
    if (i >= (long long)J.w * J.h) return;
    const int y = (int)(i / J.w), x = (int)(i - (long long)y * J.w);
    const long long f = blockIdx.y;
    const int lo = J.ay.bounds[2 * y], n = J.ay.bounds[2 * y + 1];
    if (FMT == RESIZE_RGB8) {
        const int* kk = J.ay.ki + (long long)y * J.ay.ksize;
        int r = 1 << (SGS_RESIZE_BITS - 1), g = r, b = r;
        if (J.v_from_src) {
            const float* col = J.src + f * J.src_stride + ((long long)lo * J.w + x) * 3;
            for (int j = 0; j < n; ++j) {
                const float* p = col + (long long)j * J.w * 3;
                const int k = kk[j];
                r += resize_level(p[0]) * k; g += resize_level(p[1]) * k; b += resize_level(p[2]) * k;
            }
        } else {
            const unsigned* col = J.mid + f * J.H * J.w + (long long)lo * J.w + x;
            for (int j = 0; j < n; ++j) {
                const unsigned p = col[(long long)j * J.w];
                const int k = kk[j];
                r += (int)(p & 255u) * k; g += (int)((p >> 8) & 255u) * k; b += (int)((p >> 16) & 255u) * k;
            }
        }
        resize_store_rgb(J.dst + f * J.dst_stride + 3 * i, resize_clamp8(r), resize_clamp8(g), resize_clamp8(b));
    } else {
        const double* kd = J.ay.kd + (long long)y * J.ay.ksize;
        double s = 0.0;
        if (J.v_from_src) {
            const float* col = J.src + f * J.src_stride + (long long)lo * J.w + x;
            for (int j = 0; j < n; ++j) s = s + (double)resize_clip(col[(long long)j * J.w], J.clip_lo, J.clip_hi) * kd[j];
        } else {
            const unsigned* col = J.mid + f * J.H * J.w + (long long)lo * J.w + x;
            for (int j = 0; j < n; ++j) s = s + (double)__uint_as_float(col[(long long)j * J.w]) * kd[j];
        }
        J.dst[f * J.dst_stride + i] = (float)s;
    }
}

// Both passes skipped: the quantised (RGB8) or clipped (F32) frame itself.
template <int FMT>
__global__ __launch_bounds__(SGS_RESIZE_THREADS) void k_resize_copy(ResizeJob J) {
    const long long i = (long long)blockIdx.x * SGS_RESIZE_THREADS + threadIdx.x;
    if (i >= (long long)J.w * J.h) return;
    const long long f = blockIdx.y;
    if (FMT == RESIZE_RGB8) {
        const float* p = J.src + f * J.src_stride + 3 * i;
        resize_store_rgb(J.dst + f * J.dst_stride + 3 * i, (unsigned)resize_level(p[0]), (unsigned)resize_level(p[1]), (unsigned)resize_level(p[2]));
    } else {
        J.dst[f * J.dst_stride + i] = resize_clip(J.src[f * J.src_stride + i], J.clip_lo, J.clip_hi);
    }
}

// The first source index and the numerator of the weight of the second, of output o on an axis of `in` -> `out` samples: the exact
// position ((2o + 1) in - out) / 2 out, not below 0 and, from the last sample on, the last sample itself.
__device__ __forceinline__ void resize_linear_tap(int o, int in, int out, int& i0, int& i1, long long& frac) {
    long long s = (2ll * o + 1) * in - out;
    if (s < 0) s = 0;
    const long long den = 2ll * out;
    long long q = s / den;
    frac = s - q * den;
    if (q >= in - 1) { q = in - 1; frac = 0; i1 = (int)q; }
    else i1 = (int)q + 1;
    i0 = (int)q;
}

// Bilinear at half-pixel centres: [H, W] -> [h, w] in one launch.
template <int FMT>
__global__ __launch_bounds__(SGS_RESIZE_THREADS) void k_resize_linear(ResizeJob J) {
    const long long i = (long long)blockIdx.x * SGS_RESIZE_THREADS + threadIdx.x;
    if (i >= (long long)J.w * J.h) return;
    const int y = (int)(i / J.w), x = (int)(i - (long long)y * J.w);
    const long long f = blockIdx.y;
    int x0, x1, y0, y1;
    long long fx, fy;
    resize_linear_tap(x, J.W, J.w, x0, x1, fx);
    resize_linear_tap(y, J.H, J.h, y0, y1, fy);
    const long long dx = 2ll * J.w, dy = 2ll * J.h;
    if (FMT == RESIZE_RGB8) {
        const float* img = J.src + f * J.src_stride;
        const float *a = img + ((long long)y0 * J.W + x0) * 3, *b = img + ((long long)y0 * J.W + x1) * 3,
                    *c = img + ((long long)y1 * J.W + x0) * 3, *d = img + ((long long)y1 * J.W + x1) * 3;
        const long long wa = (dx - fx) * (dy - fy), wb = fx * (dy - fy), wc = (dx - fx) * fy, wd = fx * fy, den = dx * dy;
        unsigned out[3];
        for (int ch = 0; ch < 3; ++ch) {
            const long long s = resize_level(a[ch]) * wa + resize_level(b[ch]) * wb + resize_level(c[ch]) * wc + resize_level(d[ch]) * wd;
            out[ch] = (unsigned)((unsigned long long)(s + (den >> 1)) / (unsigned long long)den);
        }
        resize_store_rgb(J.dst + f * J.dst_stride + 3 * i, out[0], out[1], out[2]);
    } else {
        const float* img = J.src + f * J.src_stride;
        const float a = resize_clip(img[(long long)y0 * J.W + x0], J.clip_lo, J.clip_hi), b = resize_clip(img[(long long)y0 * J.W + x1], J.clip_lo, J.clip_hi),
                    c = resize_clip(img[(long long)y1 * J.W + x0], J.clip_lo, J.clip_hi), d = resize_clip(img[(long long)y1 * J.W + x1], J.clip_lo, J.clip_hi);
        const float tx = (float)fx / (float)dx, ty = (float)fy / (float)dy;
        const float top = a + (b - a) * tx, bot = c + (d - c) * tx;
        J.dst[f * J.dst_stride + i] = top + (bot - top) * ty;
    }
}

// ---- host side: the tap table of one axis -----------------------------------------------------------------------------------------
namespace resize {

struct AxisTable {
    int ksize = 0;
    std::vector<int> bounds;               // [out][2]
    std::vector<int> ki;                   // RGB8
    std::vector<double> kd;                // F32
};

inline double cubic(double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// The windows and normalised weights of `in` -> `out` samples, all in fp64 with multiply and add unfused; fixed: also the RGB8 weights.
inline void build_axis(int in, int out, bool fixed, AxisTable& T) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double ss = 1.0 / fs;                // (the argument is multiplied by the reciprocal, as Pillow does: not the same bits as a division)
    T.ksize = (int)std::ceil(support) * 2 + 1;
    T.bounds.assign((size_t)out * 2, 0);
    std::vector<double> k((size_t)out * T.ksize, 0.0);
    for (int o = 0; o < out; ++o) {
        const double c = (o + 0.5) * scale;
        int lo = (int)(c - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(c + support + 0.5);
        if (hi > in) hi = in;
        const int n = hi - lo;
        double* kk = &k[(size_t)o * T.ksize];
        double ww = 0.0;
        for (int j = 0; j < n; ++j) {
            const double w = cubic((j + lo - c + 0.5) * ss);
            kk[j] = w;
            ww = ww + w;
        }
        for (int j = 0; j < n; ++j)
            if (ww != 0.0) kk[j] = kk[j] / ww;
        T.bounds[2 * o] = lo; T.bounds[2 * o + 1] = n;
    }
    if (fixed) {
        T.ki.resize(k.size());
        for (size_t j = 0; j < k.size(); ++j)
            T.ki[j] = (int)(k[j] * (double)(1 << SGS_RESIZE_BITS) + (k[j] >= 0.0 ? 0.5 : -0.5));
    } else {
        T.kd.swap(k);
    }
}

}  // namespace resize
}  // namespace sgs
