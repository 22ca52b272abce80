// sgs_jpeg.h — gfx950 kernels of the baseline JPEG encoder (sgs_encode_jpeg, include/sage_gs.h).
//
// Written from ITU-T T.81 (baseline sequential DCT, Huffman, 8 bit; the Annex K tables) and the JFIF colour convention.  The reference
// has no encoder of its own: it hands uint8 frames to PIL (generate_images.py:431-432; vlm_client_modular.py:346-351).
//
// A call of n frames is three stream-ordered launches with no host synchronisation in between:
//   k_jpeg_intervals<false>  one wave per restart interval: levels, YCbCr, subsampling, DCT, quantiser, Huffman coding into an LDS bit
//                            buffer, 0xFF count — writes only the interval's stuffed byte length
//   k_jpeg_scan              one workgroup: place_files (sgs_encode.h) over (length + 2 marker bytes [+ header]) of every interval of
//                            every frame -> the absolute offset of every interval in `out`, the total, the status words
//   k_jpeg_intervals<true>   the same wave codes the same interval again and writes header / stuffed bytes / RSTn or EOI where the scan
//                            put them; a frame whose end lies beyond the capacity is not written at all
// Coding an interval twice saves the worst-case slot per interval a one-pass coder would need (19 898 bytes for 48 blocks, 7.6 MB a
// frame) plus the copy out of it; what the library owns is 12 bytes per interval.  What the second pass costs is in
// profiles/jpeg_encode_bench.json (scripts/jpeg_encode_bench.py: the encode alone, per frame and per batch of 64).
//
// A restart interval is SGS_JPEG_BLOCKS = 48 blocks: 8 MCUs of 4:2:0 (4 Y + Cb + Cr each) or 16 MCUs of 4:4:4.  Every interval starts
// byte-aligned with DC predictors of 0 (T.81 E.1.4 / F.1.1.5), so a wave needs nothing from its neighbours, and the bytes of an interval
// depend on the frame's pixels alone: a frame's file is the same bit for bit however it is issued.
//
// Lanes: one lane per sample for loading and the row pass, one lane per zigzag position for the column pass, the quantiser and the
// entropy coder.  Run lengths come from one ballot of the non-zero positions (the distance to the next lower set bit), every lane forms
// its own bit string (<= 3 ZRL + code + amplitude = 59 bits), a wave prefix sum of the lengths places it, and lanes OR their pieces into
// the LDS bit buffer.  Byte stuffing is a second sweep: ballot of the 0xFF bytes, popcount below the lane = the shift of each byte.
//
// From the 8-bit levels on, fp32 arithmetic is written with explicit fmaf and single operations only (no a * b + c for a compiler to
// contract or not), so the host compiler of the CPU test build and hipcc produce the same bits from the same levels.  The level itself
// (jpeg_level) is k_pack_rgba8's expression, x * 255 + 0.5, on purpose — the file must show the picture that kernel packs — and that one
// hipcc fuses and the host compiler does not: an input within an ulp of a level boundary may become another level in the two builds.
#pragma once
#include <cmath>

#include "sgs_common.h"
#include "sgs_encode.h"

#define SGS_JPEG_BLOCKS 48                 // 8x8 blocks per restart interval
#define SGS_JPEG_BLOCK_BITS 1658           // most bits a block can take: DC 9 + 11, 63 x (AC code 16 + amplitude 10)
#define SGS_JPEG_INT_BYTES ((SGS_JPEG_BLOCKS * SGS_JPEG_BLOCK_BITS + 7) / 8)       // 9948: an interval before stuffing
#define SGS_JPEG_LDS_WORDS 2560            // >= INT_BYTES / 4 + 64 (zeroed 64 words at a time, ahead of the write position): 10 KiB
#define SGS_JPEG_HEADER 629                // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 2 x 33 + 2 x 183, DRI 6, SOS 14
#define SGS_JPEG_SCAN_THREADS 256

namespace sgs {

struct JpegTables {                        // one device copy per (width, height, quality, subsampling)
    float q[2][64];                        // quantiser steps by zigzag position (0 luminance, 1 chrominance)
    float scale[64];                       // c(u) c(v) / 4 by zigzag position (T.81 A.3.3; 1/8 exactly at DC)
    float cosm[64];                        // [u][x] = cos((2x + 1) u pi / 16)
    unsigned hdc[2][12];                   // code << 8 | length, by size category
    unsigned hac[2][256];                  // code << 8 | length, by run << 4 | size
    unsigned char nat[64];                 // natural index (v * 8 + u) of zigzag position k
    unsigned char header[SGS_JPEG_HEADER + 3];
};

struct JpegJob {
    const float* rgb;                      // n_frames frames, frame_stride floats apart
    long long frame_stride;
    int width, height;
    int s420;                              // 1: 4:2:0 (16x16-pixel MCUs of 6 blocks), 0: 4:4:4 (8x8-pixel MCUs of 3)
    int mcus_x, n_mcu;                     // MCUs per row, per frame
    int ri;                                // MCUs per restart interval
    int n_int;                             // intervals per frame
    int n_frames;
    const JpegTables* tab;
    unsigned* sizes;                       // [n_frames * n_int] stuffed bytes of each interval
    FileSink sink;                         // offs: [n_frames * n_int + 1] where each interval's data starts in out (interval 0: its header)
};

// An 8-bit level as k_pack_rgba8 makes it.
__device__ __forceinline__ float jpeg_level(float x) {
    const float c = fminf(fmaxf(x, 0.f), 1.f);
    return (float)(unsigned)(c * 255.0f + 0.5f);
}

// One restart interval per 64-lane workgroup.  WRITE = false: only sizes[]; WRITE = true: the bytes, at offs[].
template <bool WRITE>
__global__ __launch_bounds__(64) void k_jpeg_intervals(JpegJob J) {
    __shared__ unsigned s_bits[SGS_JPEG_LDS_WORDS];
    __shared__ float s_blk[64], s_tmp[64];
    __shared__ float s_drg[256], s_dbg[256];               // R - G and B - G levels of a 16x16 MCU (4:2:0 chroma is their 2x2 mean)
    __shared__ float s_q[2][64], s_scale[64], s_cos[64];
    __shared__ unsigned s_hdc[2][12], s_hac[2][256];
    __shared__ unsigned char s_nat[64];

    const int lane = (int)threadIdx.x;
    const long long gidx = (long long)blockIdx.x;
    const int frame = (int)(gidx / J.n_int), it = (int)(gidx % J.n_int);
    unsigned char* dst = nullptr;
    if (WRITE) {
        long long at;
        if (!file_unit_offset(J.sink, gidx, J.n_int, lane == 0, at)) return;
        if (it == 0) {
            for (int i = lane; i < SGS_JPEG_HEADER; i += 64) J.sink.out[at + i] = J.tab->header[i];
            at += SGS_JPEG_HEADER;
        }
        dst = J.sink.out + at;
    }
    s_q[0][lane] = J.tab->q[0][lane]; s_q[1][lane] = J.tab->q[1][lane];
    s_scale[lane] = J.tab->scale[lane]; s_cos[lane] = J.tab->cosm[lane]; s_nat[lane] = J.tab->nat[lane];
    for (int i = lane; i < 256; i += 64) { s_hac[0][i] = J.tab->hac[0][i]; s_hac[1][i] = J.tab->hac[1][i]; }
    if (lane < 12) { s_hdc[0][lane] = J.tab->hdc[0][lane]; s_hdc[1][lane] = J.tab->hdc[1][lane]; }
    s_bits[lane] = 0u;
    int zeroed = 64;
    __syncthreads();

    const float* img = J.rgb + (long long)frame * J.frame_stride;
    const int bpm = J.s420 ? 6 : 3;
    const int y8 = lane >> 3, x8 = lane & 7;
    const int nat = s_nat[lane], cu = nat & 7, cv = nat >> 3;
    int pred_y = 0, pred_cb = 0, pred_cr = 0;              // DC predictors: 0 at the start of every restart interval
    unsigned bitpos = 0;
    float rg = 0.f, bg = 0.f;                              // 4:4:4: this lane's pixel, kept from the Y block for Cb and Cr

    for (int b = 0; b < SGS_JPEG_BLOCKS; ++b) {
        const int m = it * J.ri + b / bpm, sub = b % bpm;
        if (m >= J.n_mcu) break;
        const int mx = m % J.mcus_x, my = m / J.mcus_x;
        const int comp = J.s420 ? (sub < 4 ? 0 : sub - 3) : sub;
        float s;
        if (comp == 0) {
            const int px = J.s420 ? mx * 16 + (sub & 1) * 8 + x8 : mx * 8 + x8;
            const int py = J.s420 ? my * 16 + (sub >> 1) * 8 + y8 : my * 8 + y8;
            const float* p = img + 3ll * ((long long)min(py, J.height - 1) * J.width + min(px, J.width - 1));   // replicate the last column / row
            const float r = jpeg_level(p[0]), g = jpeg_level(p[1]), bl = jpeg_level(p[2]);
            rg = r - g; bg = bl - g;                       // exact (integers)
            // the JFIF matrix with its rows' sums (1, 0, 0) taken out: Y = G + 0.299 (R - G) + 0.114 (B - G); greys are exact
            s = fmaf(0.299f, rg, fmaf(0.114f, bg, g - 128.0f));
            if (J.s420) {
                const int at = ((sub >> 1) * 8 + y8) * 16 + (sub & 1) * 8 + x8;
                s_drg[at] = rg; s_dbg[at] = bg;
            }
        } else {
            float srg = rg, sbg = bg, w = 1.0f;
            if (J.s420) {                                  // (the Y blocks' stores are behind their barriers)
                const int at = (2 * y8) * 16 + 2 * x8;
                srg = (s_drg[at] + s_drg[at + 1]) + (s_drg[at + 16] + s_drg[at + 17]);      // exact (integers): the mean is one scaling
                sbg = (s_dbg[at] + s_dbg[at + 1]) + (s_dbg[at + 16] + s_dbg[at + 17]);
                w = 0.25f;
            }
            // Cb = -0.168736 (R - G) + 0.5 (B - G); Cr = 0.5 (R - G) - 0.081312 (B - G)
            s = comp == 1 ? w * fmaf(-0.168736f, srg, 0.5f * sbg) : w * fmaf(-0.081312f, sbg, 0.5f * srg);
        }
        // 8x8 DCT-II: rows (lane = y, u), then columns with lane = zigzag position
        s_blk[lane] = s;
        __syncthreads();
        float a = s_blk[y8 * 8] * s_cos[x8 * 8];
#pragma unroll
        for (int x = 1; x < 8; ++x) a = fmaf(s_blk[y8 * 8 + x], s_cos[x8 * 8 + x], a);
        s_tmp[lane] = a;                                   // [y][u]
        __syncthreads();
        float f = s_cos[cv * 8] * s_tmp[cu];
#pragma unroll
        for (int y = 1; y < 8; ++y) f = fmaf(s_cos[cv * 8 + y], s_tmp[y * 8 + cu], f);
        f = f * s_scale[lane];
        const int tq = comp ? 1 : 0;
        int c = (int)roundf(f / s_q[tq][lane]);            // one rounding, halves away from zero
        if (lane > 0) c = c < -1023 ? -1023 : c > 1023 ? 1023 : c;      // (the AC alphabet ends at size 10; |F| < 1024 for 8-bit input anyway)

        // entropy coding: this lane's symbol(s)
        const int dc = __shfl(c, 0);
        const int val = lane == 0 ? c - (comp == 0 ? pred_y : comp == 1 ? pred_cb : pred_cr) : c;
        if (comp == 0) pred_y = dc; else if (comp == 1) pred_cb = dc; else pred_cr = dc;
        const int mag = val < 0 ? -val : val;
        const int size = mag ? 32 - __clz(mag) : 0;
        const unsigned amp = (unsigned)(val + (val >> 31)) & ((1u << size) - 1u);
        const unsigned long long nz = __ballot(lane > 0 && c != 0);
        unsigned long long code = 0;
        unsigned len = 0;
        if (lane == 0) {
            const unsigned h = s_hdc[tq][size];
            code = ((unsigned long long)(h >> 8) << size) | amp;
            len = (h & 255u) + (unsigned)size;
        } else if (c != 0) {
            const unsigned long long below = nz & ((1ull << lane) - 1ull);
            const int prev = below ? 63 - __clzll((long long)below) : 0;
            const int run = lane - prev - 1;
            const unsigned zrl = s_hac[tq][0xF0];
            for (int i = 0; i < (run >> 4); ++i) { code = (code << (zrl & 255u)) | (zrl >> 8); len += zrl & 255u; }
            const unsigned h = s_hac[tq][((run & 15) << 4) | size];
            code = (((code << (h & 255u)) | (h >> 8)) << size) | amp;
            len += (h & 255u) + (unsigned)size;
        } else if (lane == 63) {                           // the block ends in zeros: EOB
            const unsigned h = s_hac[tq][0];
            code = h >> 8; len = h & 255u;
        }
        unsigned incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const unsigned total = __shfl(incl, 63);
        const int need = (int)((bitpos + total + 31u) >> 5) + 1;
        while (zeroed < need) { s_bits[zeroed + lane] = 0u; zeroed += 64; }
        __syncthreads();
        if (len) {
            const unsigned p = bitpos + incl - len, o = p & 31u;
            const unsigned long long v = code << (64u - len);                  // left-aligned
            const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
            const unsigned w0 = hi >> o, w1 = o ? (hi << (32u - o)) | (lo >> o) : lo, w2 = o ? lo << (32u - o) : 0u;
            if (w0) atomicOr(&s_bits[p >> 5], w0);
            if (w1) atomicOr(&s_bits[(p >> 5) + 1], w1);
            if (w2) atomicOr(&s_bits[(p >> 5) + 2], w2);
        }
        bitpos += total;
    }
    // pad the last byte with ones (T.81 F.1.2.3), then stuff
    if (lane == 0 && (bitpos & 7u)) {
        const unsigned pad = 8u - (bitpos & 7u);
        atomicOr(&s_bits[bitpos >> 5], ((1u << pad) - 1u) << (32u - (bitpos & 31u) - pad));
    }
    __syncthreads();
    const unsigned nbytes = (bitpos + 7u) >> 3;
    unsigned outpos = 0;
    for (unsigned base = 0; base < nbytes; base += 64) {
        const unsigned i = base + (unsigned)lane;
        const bool valid = i < nbytes;
        const unsigned byte = valid ? (s_bits[i >> 2] >> (24u - 8u * (i & 3u))) & 255u : 0u;
        const bool ff = valid && byte == 255u;
        const unsigned long long mff = __ballot(ff);
        if (WRITE && valid) {
            const unsigned at = outpos + (unsigned)lane + (unsigned)__popcll(mff & ((1ull << lane) - 1ull));
            dst[at] = (unsigned char)byte;
            if (ff) dst[at + 1] = 0;
        }
        outpos += min(64u, nbytes - base) + (unsigned)__popcll(mff);
    }
    if (lane == 0) {
        if (WRITE) {
            dst[outpos] = 0xFF;
            dst[outpos + 1] = (unsigned char)(it == J.n_int - 1 ? 0xD9 : 0xD0 + (it & 7));      // EOI / RSTn, n cycling 0..7
        } else {
            J.sizes[gidx] = outpos;
        }
    }
}

// place_files over every interval of every frame of (stuffed bytes + 2 marker bytes + the header at a frame's first interval).
__global__ __launch_bounds__(SGS_JPEG_SCAN_THREADS) void k_jpeg_scan(JpegJob J) {
    __shared__ unsigned long long s_part[SGS_JPEG_SCAN_THREADS];
    place_files<SGS_JPEG_SCAN_THREADS>(J.sink, (long long)J.n_frames * J.n_int, s_part, [&J](long long i) {
        return (unsigned long long)J.sizes[i] + 2ull + (i % J.n_int == 0 ? (unsigned long long)SGS_JPEG_HEADER : 0ull);
    });
}

// ---- host side: the tables of T.81 Annex K and the file header ---------------------------------------------------------------------
namespace jpeg {

// K.1 / K.2, natural order
static const unsigned char kQLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                        14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const unsigned char kQChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                        47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Figure A.6: natural index of zigzag position k
static const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// K.3 - K.6: BITS (codes of each length 1..16) and HUFFVAL
static const unsigned char kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const unsigned char kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static const unsigned char kAcLumVals[162] = {
    1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
    193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
    56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
    115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
    212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
static const unsigned char kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static const unsigned char kAcChrVals[162] = {
    0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
    9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
    55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
    210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};

// T.81 Annex C: canonical codes from BITS / HUFFVAL, stored as code << 8 | length at the symbol's index.
inline void huff_codes(const unsigned char* bits, const unsigned char* vals, unsigned* out, int n_out) {
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) out[vals[k]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
}

// The IJG quality rule: 5000 / q below 50, 200 - 2 q from 50 on; (t * s + 50) / 100 clamped to 1..255.
inline int quant_step(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * s + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

inline unsigned char* put_dht(unsigned char* p, int tc_th, const unsigned char* bits, const unsigned char* vals, int n) {
    *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = (unsigned char)(19 + n); *p++ = (unsigned char)tc_th;
    for (int i = 0; i < 16; ++i) *p++ = bits[i];
    for (int i = 0; i < n; ++i) *p++ = vals[i];
    return p;
}

inline void build_tables(JpegTables& T, int width, int height, int quality, bool s420, int ri) {
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < 64; ++k) {
        const int n = kZigzag[k], u = n & 7, v = n >> 3;
        T.nat[k] = (unsigned char)n;
        T.q[0][k] = (float)quant_step(kQLum[n], quality);
        T.q[1][k] = (float)quant_step(kQChr[n], quality);
        T.scale[k] = (float)((u ? 1.0 : std::sqrt(0.5)) * (v ? 1.0 : std::sqrt(0.5)) * 0.25);
        T.cosm[k] = (float)std::cos((2 * (k & 7) + 1) * (k >> 3) * pi / 16.0);
    }
    T.scale[0] = 0.125f;
    huff_codes(kDcLumBits, kDcVals, T.hdc[0], 12);
    huff_codes(kDcChrBits, kDcVals, T.hdc[1], 12);
    huff_codes(kAcLumBits, kAcLumVals, T.hac[0], 256);
    huff_codes(kAcChrBits, kAcChrVals, T.hac[1], 256);
    unsigned char* p = T.header;
    const unsigned char app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (unsigned char c : app0) *p++ = c;
    for (int t = 0; t < 2; ++t) {
        *p++ = 0xFF; *p++ = 0xDB; *p++ = 0; *p++ = 67; *p++ = (unsigned char)t;
        for (int k = 0; k < 64; ++k) *p++ = (unsigned char)T.q[t][k];
    }
    const unsigned char sof[] = {0xFF, 0xC0, 0, 17, 8, (unsigned char)(height >> 8), (unsigned char)height, (unsigned char)(width >> 8),
                                 (unsigned char)width, 3, 1, (unsigned char)(s420 ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
    for (unsigned char c : sof) *p++ = c;
    p = put_dht(p, 0x00, kDcLumBits, kDcVals, 12);
    p = put_dht(p, 0x10, kAcLumBits, kAcLumVals, 162);
    p = put_dht(p, 0x01, kDcChrBits, kDcVals, 12);
    p = put_dht(p, 0x11, kAcChrBits, kAcChrVals, 162);
    const unsigned char tail[] = {0xFF, 0xDD, 0, 4, (unsigned char)(ri >> 8), (unsigned char)ri,
                                  0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (unsigned char c : tail) *p++ = c;
    static_assert(sizeof app0 + 2 * 69 + sizeof sof + 2 * 33 + 2 * 183 + sizeof tail == SGS_JPEG_HEADER, "header length");
}

}  // namespace jpeg
}  // namespace sgs
