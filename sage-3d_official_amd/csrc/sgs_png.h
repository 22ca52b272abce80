// sgs_png.h — gfx950 kernels of the PNG encoder (sgs_encode_png, include/sage_gs.h).
//
// Written from the PNG specification (ISO/IEC 15948: signature, IHDR / IDAT / IEND, the five filters, CRC-32), RFC 1950 (zlib framing,
// Adler-32) and RFC 1951 (deflate: stored and dynamic-Huffman blocks).  The reference has no encoder of its own: it hands arrays to PIL
// (vlm_client_modular.py:354-365; simple_env.py:2757-2759).
//
// The image is cut into strips: as many whole rows as fit SGS_PNG_STRIP filtered bytes (at least one).  A call of n frames is three
// stream-ordered launches with no host synchronisation in between:
//   k_png_strips   one 64-lane workgroup per strip: samples, filter choice per row, Adler-32 partial sums, run matching, histogram,
//                  length-limited Huffman tables, the deflate bits into an LDS buffer, CRC-32 — the finished chunk body ("IDAT" + data)
//                  goes to the strip's slot of the library's scratch (stored-size slots: a strip is never longer than stored)
//   k_png_scan     one workgroup: place_files (sgs_encode.h) over the chunk sizes of every strip of every frame -> the absolute offset
//                  of every chunk in `out`, the total, the status words; the Adler-32 of each frame from its strips' (a, b) pairs
//   k_png_gather   one workgroup per strip copies the slot to where the scan put it and writes the framing: signature + IHDR before a
//                  frame's first chunk, length and CRC around each, final block + Adler-32 + IEND after its last
// Coding once into slots rather than twice around the scan (sgs_jpeg.h's shape): a strip's work is several sweeps over 16 KiB plus a
// serial table construction, and its slot is bounded by the stored size (the strip + 16 bytes), so a second coding pass would cost
// more than the copy it saves.
//
// A strip depends on nothing outside it but the raw row above its first row (read from the input): its deflate blocks match no
// further back than the strip's first byte and end byte-aligned on an empty stored block, and its IDAT chunk's CRC covers its own
// bytes.  A frame's file is therefore the same bit for bit however it is issued.
//
// Everything after the samples is integer arithmetic: the host compiler of the CPU test build and hipcc produce the same file from the
// same samples.  The 8-bit level is k_pack_rgba8's expression (x * 255 + 0.5, which hipcc fuses and the host compiler does not); the
// 16-bit depth sample is one fp32 multiply and a truncation, with nothing to contract.
#pragma once
#include <cmath>

#include "sgs_common.h"
#include "sgs_encode.h"

#define SGS_PNG_STRIP 16384                // filtered bytes per strip (and the longest filtered row)
#define SGS_PNG_OUT_WORDS 4112             // "IDAT" 4 + zlib header 2 + stored header 5 + strip + alignment block 5 = 16 400 B, + 2 spill words, rounded up
#define SGS_PNG_SYMS 288                   // literal / length alphabet (286 used)
#define SGS_PNG_HEAD 33                    // signature 8 + IHDR chunk 25
#define SGS_PNG_SCAN_THREADS 256
#define SGS_PNG_GATHER_THREADS 256
#define SGS_PNG_POLY 0xEDB88320u           // CRC-32, reflected
#define SGS_PNG_ADLER 65521u

namespace sgs {

struct PngStripRec {
    unsigned len;                          // bytes in the slot: "IDAT" + the chunk's data (without a last chunk's final block and Adler-32)
    unsigned crc;                          // CRC-32 register over them (before the final complement)
    unsigned a, b;                         // sum f[i] and sum (S - i) f[i] over the strip's S filtered bytes, mod 65521
};

struct PngJob {
    const float* src;                      // n_frames frames, frame_stride floats apart
    long long frame_stride;
    int width, height;
    int depth16;                           // 0: fp32 [H,W,3] -> 8-bit RGB; 1: fp32 [H,W] metres -> 16-bit grey
    float scale, dmax;
    int bpp, row_bytes;                    // bytes per pixel, per raw row
    int rows_per_strip, n_strips, n_frames;
    long long slot;                        // bytes between strip slots
    unsigned char* slots;
    PngStripRec* rec;                      // [n_frames * n_strips]
    unsigned* adler;                       // [n_frames]
    FileSink sink;                         // offs: [n_frames * n_strips + 1] where each strip's chunk starts in out (strip 0: the signature)
    unsigned char head[SGS_PNG_HEAD + 3];
};

// Byte x of raw row `row` (the filter-type byte not counted).
__device__ __forceinline__ unsigned png_sample(const PngJob& J, const float* img, int row, int x) {
    if (J.depth16) {
        const float d = img[(long long)row * J.width + (x >> 1)];
        const float c = fminf(fmaxf(d, 0.f), J.dmax);      // NaN -> 0 (fmaxf returns the other operand)
        const float m = c * J.scale;                       // one multiply: NumPy's clip(d, 0, max) * scale
        const unsigned v = (unsigned)m;                    // truncation: astype(uint16)
        return (x & 1) ? (v & 255u) : (v >> 8);            // big-endian
    }
    const float c = fminf(fmaxf(img[(long long)row * J.row_bytes + x], 0.f), 1.f);
    return (unsigned)(c * 255.0f + 0.5f);                  // k_pack_rgba8's level
}

__device__ __forceinline__ int png_sabs(unsigned f) { return f < 128u ? (int)f : 256 - (int)f; }     // |byte read as signed|

__device__ __forceinline__ unsigned png_paeth(unsigned a, unsigned b, unsigned c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// Product of two polynomials mod the CRC-32 polynomial, reflected bit order (x^0 = 0x80000000).
__device__ __forceinline__ unsigned png_gfmul(unsigned a, unsigned b) {
    unsigned p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ SGS_PNG_POLY : b >> 1;
    }
    return p;
}

// The literal / length symbol of a match length 3..258, its extra bits and their count.
__device__ __forceinline__ unsigned png_len_sym(unsigned len, unsigned& extra, unsigned& nextra) {
    extra = 0; nextra = 0;
    if (len == 258u) return 285u;
    const unsigned l = len - 3u;
    if (l < 8u) return 257u + l;
    const unsigned e = (unsigned)(31 - __clz((int)l)) - 2u;
    nextra = e; extra = l & ((1u << e) - 1u);
    return 257u + 4u * e + 4u + ((l >> e) & 3u);
}

// The tokens of one window of 64 positions of the strip's filtered bytes f[0..S): lane = position base + lane.  Matches are runs
// (distance 1) of 3..258 bytes, parsed greedily from the run's first repeated byte, as zlib's Z_RLE strategy does.  A run is coded by
// the lane of its last byte once its length is known; `carry` is the length of a run that reaches the window from before and is not
// coded yet (below 258: the lane of the window's last byte codes a full match whenever that much has gathered).  A token is a literal
// 0..255 or 256 + match length; a lane has at most three (t0, t1, t2 in stream order).
__device__ __forceinline__ unsigned png_window_tokens(const unsigned char* f, int S, int base, int lane, unsigned& carry, unsigned& t0, unsigned& t1,
                                                      unsigned& t2) {
    const int i = base + lane;
    const bool valid = i < S;
    const unsigned me = valid ? f[i] : 0u;
    const bool cur = valid && i >= 1 && f[i - 1] == me;
    const bool nxt = i + 1 < S && f[i + 1] == me;
    const unsigned long long m = __ballot(cur);
    unsigned n = 0, pending = 0;
    t0 = t1 = t2 = 0;
    if (cur) {
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);
        unsigned T = below ? (unsigned)(lane - 63 + __clzll((long long)below)) : carry + (unsigned)lane + 1u;
        if (!nxt) {                                        // the run ends here
            if (T >= 258u) { t0 = 256u + 258u; n = 1; T -= 258u; }
            if (T >= 3u) {
                if (n) t1 = 256u + T; else t0 = 256u + T;
                ++n;
            } else if (T) {                                // one or two bytes left: literals
                if (n) { t1 = me; if (T == 2u) t2 = me; } else { t0 = me; if (T == 2u) t1 = me; }
                n += T;
            }
        } else if (lane == 63) {                           // the run goes on into the next window
            if (T >= 258u) { t0 = 256u + 258u; n = 1; T -= 258u; }
            pending = T;
        }
    } else if (valid) {
        t0 = me; n = 1;
    }
    carry = __shfl(pending, 63);
    return n;
}

// Code lengths of a minimum-redundancy code in place (Moffat & Katajainen, "In-place calculation of minimum-redundancy codes", 1995):
// A[0..n) holds the frequencies in ascending order on entry and the code lengths on exit (descending).  n >= 2.
__device__ inline void png_min_redundancy(unsigned* A, int n) {
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (unsigned)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (unsigned)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
    int avbl = 1, used = 0;
    unsigned dpth = 0;
    root = n - 2; next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = dpth; --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
}

// How many codes of each length the optimal code within `limit` bits has (package-merge: Larmore & Hirschberg, "A fast algorithm for
// optimal length-limited Huffman codes", 1990), for a small alphabet: F[0..n) the frequencies in ascending order, 2 <= n <= 32,
// n <= 2^limit.  Level by level from the deepest, the items of a level are the leaves merged with the pairs of the level below (the
// 2n - 2 cheapest are kept; a bit mask per level records which are leaves); going back from the top, a leaf among the items taken at a
// level adds one bit to its symbol — always the rarest symbols first, so only the count per level is needed.  work: 256 words.
__device__ inline void png_package_merge(const unsigned* F, int n, int limit, unsigned* num, unsigned* work) {
    unsigned* prev = work, *cur = work + 64, *mask = work + 128, *len = work + 176;      // mask[2 lev], mask[2 lev + 1]
    const int keep = 2 * n - 2;
    int np = n;
    for (int i = 0; i < n; ++i) { prev[i] = F[i]; len[i] = 0; }
    mask[2 * limit] = n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; mask[2 * limit + 1] = 0;
    for (int lev = limit - 1; lev >= 1; --lev) {
        const int npk = np >> 1;
        int a = 0, b = 0, t = 0;
        unsigned m0 = 0, m1 = 0;
        while (t < keep && (a < n || b < npk)) {
            const unsigned pw = b < npk ? prev[2 * b] + prev[2 * b + 1] : 0xFFFFFFFFu;
            if (a < n && F[a] <= pw) {
                cur[t] = F[a++];
                if (t < 32) m0 |= 1u << t; else m1 |= 1u << (t - 32);
            } else { cur[t] = pw; ++b; }
            ++t;
        }
        mask[2 * lev] = m0; mask[2 * lev + 1] = m1;
        np = t;
        unsigned* sw = prev; prev = cur; cur = sw;
    }
    int need = keep;
    for (int lev = 1; lev <= limit && need > 0; ++lev) {
        const unsigned lo = need >= 32 ? 0xFFFFFFFFu : (1u << need) - 1u, hi = need > 32 ? (need >= 64 ? 0xFFFFFFFFu : (1u << (need - 32)) - 1u) : 0u;
        const int leaves = __popcll(((unsigned long long)(mask[2 * lev + 1] & hi) << 32) | (mask[2 * lev] & lo));
        for (int i = 0; i < leaves && i < n; ++i) len[i]++;
        need = 2 * (need - leaves);
    }
    for (int i = 0; i <= limit; ++i) num[i] = 0;
    for (int i = 0; i < n; ++i) num[len[i]]++;
}

// Code lengths limited to `limit` bits and canonical codes for the n used symbols sym[0..n) whose frequencies A[0..n) are in ascending
// order: lengths of the optimal code, lengths beyond the limit folded into it and the Kraft sum repaired by lengthening the deepest
// shorter codes (the construction small deflaters use), the longest lengths to the rarest symbols.  Given `work` (n <= 32, 320 words), an
// optimal code deeper than the limit is replaced by the optimal code within it (png_package_merge) instead of being repaired.
// tab[s] = reversed code | length << 16 for every symbol of the alphabet (0 for unused ones).  n >= 2.
__device__ inline void png_build_code(unsigned* A, const unsigned short* sym, int n, int limit, unsigned* tab, int n_alphabet, unsigned* num,
                                      unsigned* work = nullptr) {
    unsigned* nextc = num + 16;                            // num[0..16), nextc[0..16): the caller's (LDS, not a private array)
    for (int i = 0; i <= 15; ++i) num[i] = 0;
    if (work) for (int i = 0; i < n; ++i) work[256 + i] = A[i];
    png_min_redundancy(A, n);
    const bool too_deep = A[0] > (unsigned)limit;          // (the lengths are in descending order)
    for (int i = 0; i < n; ++i) num[A[i] < (unsigned)limit ? A[i] : (unsigned)limit]++;
    unsigned total = 0;
    for (int i = limit; i > 0; --i) total += num[i] << (limit - i);
    if (work && too_deep) { png_package_merge(work + 256, n, limit, num, work); total = 1u << limit; }
    while (total > (1u << limit)) {
        num[limit]--;
        for (int i = limit - 1; i > 0; --i)
            if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        total--;
    }
    for (int s = 0; s < n_alphabet; ++s) tab[s] = 0;
    int j = 0;
    for (int len = limit; len >= 1; --len)
        for (unsigned k = 0; k < num[len]; ++k) tab[sym[j++]] = (unsigned)len << 16;
    unsigned code = 0;
    num[0] = 0;
    for (int len = 1; len <= limit; ++len) { code = (code + num[len - 1]) << 1; nextc[len] = code; }
    for (int s = 0; s < n_alphabet; ++s) {
        const unsigned len = tab[s] >> 16;
        if (!len) continue;
        unsigned c = nextc[len]++, r = 0;
        for (unsigned b = 0; b < len; ++b) { r = (r << 1) | (c & 1u); c >>= 1; }      // deflate packs Huffman codes from their most significant bit
        tab[s] |= r;
    }
}

__device__ __forceinline__ void png_put(unsigned* bits, unsigned& pos, unsigned v, unsigned n) {       // one lane, n <= 16
    const unsigned o = pos & 31u;
    bits[pos >> 5] |= v << o;
    if (o + n > 32u) bits[(pos >> 5) + 1] |= v >> (32u - o);
    pos += n;
}

// One strip per 64-lane workgroup.
__global__ __launch_bounds__(64) void k_png_strips(PngJob J) {
    __shared__ unsigned char s_filt[SGS_PNG_STRIP];
    __shared__ unsigned s_out[SGS_PNG_OUT_WORDS];
    __shared__ unsigned s_freq[SGS_PNG_SYMS];              // histogram of the literal / length symbols
    __shared__ unsigned s_key[SGS_PNG_SYMS];               // frequencies of the used symbols: compacted, then sorted; code lengths in the end
    __shared__ unsigned short s_sym[SGS_PNG_SYMS], s_sorted[SGS_PNG_SYMS];
    __shared__ unsigned s_tab[SGS_PNG_SYMS];               // reversed code | length << 16
    __shared__ unsigned s_crc[256];
    __shared__ unsigned short s_rle[SGS_PNG_SYMS + 32];    // the code-length sequence: symbol | extra << 8
    __shared__ unsigned s_clkey[19], s_clA[19], s_cltab[19];      // the code of the code lengths: histogram, sorted, codes
    __shared__ unsigned short s_clsym[19];
    __shared__ unsigned s_num[32];                         // png_build_code's counters
    __shared__ unsigned s_misc[4];                         // [0] bit position after the block header

    const int lane = (int)threadIdx.x;
    const long long gidx = (long long)blockIdx.x;
    const int frame = (int)(gidx / J.n_strips), st = (int)(gidx % J.n_strips);
    const float* img = J.src + (long long)frame * J.frame_stride;
    const int y0 = st * J.rows_per_strip;
    const int rows = min(J.rows_per_strip, J.height - y0);
    const int nb = J.row_bytes, rowlen = nb + 1, bpp = J.bpp;
    const int S = rows * rowlen;
    const unsigned hdr = st == 0 ? 6u : 4u;                // "IDAT" [+ the zlib header]

    for (int i = lane; i < SGS_PNG_OUT_WORDS; i += 64) s_out[i] = 0u;
    for (int i = lane; i < SGS_PNG_SYMS; i += 64) s_freq[i] = 0u;
    for (int i = lane; i < 256; i += 64) {
        unsigned c = (unsigned)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ SGS_PNG_POLY : c >> 1;
        s_crc[i] = c;
    }

    // ---- filtering: per row the filter with the least sum of |filtered byte read as signed|, ties to the lowest type ------------------
    unsigned long long ad_a = 0, ad_b = 0;
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
        for (int x = lane; x < nb; x += 64) {
            const unsigned raw = png_sample(J, img, y, x);
            const unsigned a = x >= bpp ? png_sample(J, img, y, x - bpp) : 0u;
            const unsigned b = y > 0 ? png_sample(J, img, y - 1, x) : 0u;
            const unsigned c = (y > 0 && x >= bpp) ? png_sample(J, img, y - 1, x - bpp) : 0u;
            s0 += png_sabs(raw);
            s1 += png_sabs((raw - a) & 255u);
            s2 += png_sabs((raw - b) & 255u);
            s3 += png_sabs((raw - ((a + b) >> 1)) & 255u);
            s4 += png_sabs((raw - png_paeth(a, b, c)) & 255u);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            s0 += __shfl_xor(s0, d); s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d); s3 += __shfl_xor(s3, d); s4 += __shfl_xor(s4, d);
        }
        int ft = 0, best = s0;
        if (s1 < best) { best = s1; ft = 1; }
        if (s2 < best) { best = s2; ft = 2; }
        if (s3 < best) { best = s3; ft = 3; }
        if (s4 < best) { best = s4; ft = 4; }
        const int at = r * rowlen;
        if (lane == 0) {
            s_filt[at] = (unsigned char)ft;
            ad_a += (unsigned)ft; ad_b += (unsigned long long)(S - at) * (unsigned)ft;
        }
        for (int x = lane; x < nb; x += 64) {
            const unsigned raw = png_sample(J, img, y, x);
            unsigned pred = 0;
            if (ft == 1) pred = x >= bpp ? png_sample(J, img, y, x - bpp) : 0u;
            else if (ft == 2) pred = y > 0 ? png_sample(J, img, y - 1, x) : 0u;
            else if (ft >= 3) {
                const unsigned a = x >= bpp ? png_sample(J, img, y, x - bpp) : 0u;
                const unsigned b = y > 0 ? png_sample(J, img, y - 1, x) : 0u;
                if (ft == 3) pred = (a + b) >> 1;
                else pred = png_paeth(a, b, (y > 0 && x >= bpp) ? png_sample(J, img, y - 1, x - bpp) : 0u);
            }
            const unsigned f = (raw - pred) & 255u;
            s_filt[at + 1 + x] = (unsigned char)f;
            ad_a += f; ad_b += (unsigned long long)(S - (at + 1 + x)) * f;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { ad_a += __shfl_xor(ad_a, d); ad_b += __shfl_xor(ad_b, d); }
    __syncthreads();

    // ---- histogram of the tokens ------------------------------------------------------------------------------------------------------
    unsigned carry = 0;
    for (int base = 0; base < S; base += 64) {
        unsigned t0, t1, t2;
        const unsigned n = png_window_tokens(s_filt, S, base, lane, carry, t0, t1, t2);
        for (unsigned k = 0; k < n; ++k) {
            const unsigned tk = k == 0 ? t0 : k == 1 ? t1 : t2;
            unsigned ex, nex;
            atomicAdd(&s_freq[tk < 256u ? tk : png_len_sym(tk - 256u, ex, nex)], 1u);
        }
    }
    if (lane == 0) s_freq[256] = 1u;                       // end of block
    __syncthreads();

    // ---- the used symbols in ascending order of (frequency, symbol): compaction, then a rank sort --------------------------------------
    int n_used = 0;
    for (int s0 = 0; s0 < SGS_PNG_SYMS; s0 += 64) {
        const int s = s0 + lane;
        const unsigned fr = s < SGS_PNG_SYMS ? s_freq[s] : 0u;
        const unsigned long long um = __ballot(fr != 0u);
        if (fr) {
            const int at = n_used + __popcll(um & ((1ull << lane) - 1ull));
            s_key[at] = fr; s_sym[at] = (unsigned short)s;
        }
        n_used += __popcll(um);
    }
    __syncthreads();
    unsigned my_key[5], my_rank[5], my_sym[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int j = lane + 64 * q;
        my_key[q] = 0; my_rank[q] = 0; my_sym[q] = 0;
        if (j < n_used) {
            const unsigned key = s_key[j];
            unsigned rank = 0;
            for (int k = 0; k < n_used; ++k) { const unsigned o = s_key[k]; rank += (o < key || (o == key && k < j)) ? 1u : 0u; }
            my_key[q] = key; my_rank[q] = rank; my_sym[q] = s_sym[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 5; ++q)
        if (lane + 64 * q < n_used) { s_key[my_rank[q]] = my_key[q]; s_sorted[my_rank[q]] = (unsigned short)my_sym[q]; }
    __syncthreads();

    // ---- one lane: the two codes and the block header (a few thousand steps on ~300 symbols) ------------------------------------------
    unsigned char* const out8 = reinterpret_cast<unsigned char*>(s_out);
    if (lane == 0) {
        out8[0] = 'I'; out8[1] = 'D'; out8[2] = 'A'; out8[3] = 'T';
        if (st == 0) { out8[4] = 0x78; out8[5] = 0x01; }   // zlib: deflate, 32 KiB window, fastest
        png_build_code(s_key, s_sorted, n_used, 15, s_tab, SGS_PNG_SYMS, s_num);
        int hlit = 286;
        while (hlit > 257 && !(s_tab[hlit - 1] >> 16)) --hlit;
        // the lengths of the hlit literal / length codes and of the one distance code (distance 1, one bit), run-length coded
        const int N = hlit + 1;
        for (int i = 0; i < 19; ++i) s_clkey[i] = 0;
        int nr = 0;
        for (int i = 0; i < N;) {
            const unsigned v = i < hlit ? s_tab[i] >> 16 : 1u;
            int run = 1;
            while (i + run < N && (i + run < hlit ? s_tab[i + run] >> 16 : 1u) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; s_rle[nr++] = (unsigned short)(18 | ((r - 11) << 8)); s_clkey[18]++; run -= r; }
                if (run >= 3) { s_rle[nr++] = (unsigned short)(17 | ((run - 3) << 8)); s_clkey[17]++; run = 0; }
            } else {
                s_rle[nr++] = (unsigned short)v; s_clkey[v]++; --run;
                while (run >= 3) { const int r = run < 6 ? run : 6; s_rle[nr++] = (unsigned short)(16 | ((r - 3) << 8)); s_clkey[16]++; run -= r; }
            }
            for (; run > 0; --run) { s_rle[nr++] = (unsigned short)v; s_clkey[v]++; }
        }
        // the code of the code lengths: at most 7 bits; a complete code needs two symbols
        int ncl = 0;
        for (int i = 0; i < 19; ++i) ncl += s_clkey[i] ? 1 : 0;
        if (ncl < 2) s_clkey[s_clkey[0] ? 1 : 0] = 1;
        ncl = 0;
        for (int i = 0; i < 19; ++i) {                     // insertion sort by (frequency, symbol)
            const unsigned fr = s_clkey[i];
            if (!fr) continue;
            int k = ncl++;
            while (k > 0 && s_clA[k - 1] > fr) { s_clA[k] = s_clA[k - 1]; s_clsym[k] = s_clsym[k - 1]; --k; }
            s_clA[k] = fr; s_clsym[k] = (unsigned short)i;
        }
        png_build_code(s_clA, s_clsym, ncl, 7, s_cltab, 19, s_num, s_key);      // (s_key is free: the literal / length code stands in s_tab)
        const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && !(s_cltab[order[hclen - 1]] >> 16)) --hclen;
        unsigned pos = 8u * hdr;
        png_put(s_out, pos, 4u, 3);                        // BFINAL = 0, BTYPE = 10
        png_put(s_out, pos, (unsigned)(hlit - 257), 5);
        png_put(s_out, pos, 0u, 5);                        // HDIST - 1
        png_put(s_out, pos, (unsigned)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) png_put(s_out, pos, s_cltab[order[i]] >> 16, 3);
        for (int i = 0; i < nr; ++i) {
            const unsigned sy = s_rle[i] & 255u, ex = s_rle[i] >> 8, t = s_cltab[sy];
            png_put(s_out, pos, t & 0xFFFFu, t >> 16);
            if (sy >= 16u) png_put(s_out, pos, ex, sy == 16u ? 2u : sy == 17u ? 3u : 7u);
        }
        s_misc[0] = pos;
    }
    __syncthreads();

    // ---- what the dynamic block takes, against the stored one -------------------------------------------------------------------------
    unsigned cost = 0;
    for (int s = lane; s < SGS_PNG_SYMS; s += 64) {
        const unsigned fr = s_freq[s];
        const unsigned ex = (s >= 265 && s < 285) ? (unsigned)(s - 261) >> 2 : 0u;
        cost += fr * ((s_tab[s] >> 16) + ex + (s > 256 ? 1u : 0u));            // + the one-bit distance code of every match
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) cost += __shfl_xor(cost, d);
    const unsigned head_end = s_misc[0];
    const unsigned len_dyn = ((head_end + cost + 3u + 7u) >> 3) + 4u;          // ... + the empty stored block: 3 bits, padding, 00 00 FF FF
    const unsigned len_stored = hdr + 5u + (unsigned)S + 5u;
    unsigned L;
    if (len_dyn < len_stored) {
        // ---- the tokens' bits: every lane forms the string of its tokens, a prefix sum places it ---------------------------------------
        unsigned bitpos = head_end;
        carry = 0;
        for (int base = 0; base < S; base += 64) {
            unsigned t0, t1, t2;
            const unsigned n = png_window_tokens(s_filt, S, base, lane, carry, t0, t1, t2);
            unsigned long long v = 0;
            unsigned len = 0;
            for (unsigned k = 0; k < n; ++k) {
                const unsigned tk = k == 0 ? t0 : k == 1 ? t1 : t2;
                if (tk < 256u) {
                    const unsigned t = s_tab[tk];
                    v |= (unsigned long long)(t & 0xFFFFu) << len; len += t >> 16;
                } else {
                    unsigned ex, nex;
                    const unsigned t = s_tab[png_len_sym(tk - 256u, ex, nex)];
                    v |= (unsigned long long)(t & 0xFFFFu) << len; len += t >> 16;
                    v |= (unsigned long long)ex << len; len += nex + 1u;        // extra bits, then the distance code: one 0 bit
                }
            }
            unsigned incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(incl, d);
                if (lane >= d) incl += t;
            }
            if (len) {
                const unsigned p = bitpos + incl - len, o = p & 31u;
                const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
                const unsigned w0 = lo << o, w1 = o ? (lo >> (32u - o)) | (hi << o) : hi, w2 = o ? hi >> (32u - o) : 0u;
                if (w0) atomicOr(&s_out[p >> 5], w0);
                if (w1) atomicOr(&s_out[(p >> 5) + 1], w1);
                if (w2) atomicOr(&s_out[(p >> 5) + 2], w2);
            }
            bitpos += __shfl(incl, 63);
        }
        __syncthreads();
        const unsigned eob = s_tab[256];
        unsigned end = bitpos;
        if (lane == 0) png_put(s_out, end, eob & 0xFFFFu, eob >> 16);
        const unsigned at = (bitpos + (eob >> 16) + 3u + 7u) >> 3;             // the empty stored block's 3 header bits are zeros already
        if (lane == 0) { out8[at] = 0; out8[at + 1] = 0; out8[at + 2] = 0xFF; out8[at + 3] = 0xFF; }
        L = at + 4u;
    } else {
        // ---- stored: one block (a strip is at most 16 384 bytes), then the same empty block --------------------------------------------
        if (lane == 0) {
            out8[hdr] = 0;
            out8[hdr + 1] = (unsigned char)(S & 255); out8[hdr + 2] = (unsigned char)(S >> 8);
            out8[hdr + 3] = (unsigned char)(~S & 255); out8[hdr + 4] = (unsigned char)((~S >> 8) & 255);
            const unsigned at = hdr + 5u + (unsigned)S;
            out8[at] = 0; out8[at + 1] = 0; out8[at + 2] = 0; out8[at + 3] = 0xFF; out8[at + 4] = 0xFF;
        }
        for (int i = lane; i < S; i += 64) out8[hdr + 5u + (unsigned)i] = s_filt[i];
        L = len_stored;
    }
    __syncthreads();

    // ---- CRC-32 of the L bytes: a lane per piece of c bytes (zeros ahead of the first piece change nothing in a register that starts
    // at 0; the register's start value of all ones is the first four bytes complemented), then pieces joined pairwise, the left one
    // multiplied by x^(8 * bytes to its right) ----------------------------------------------------------------------------------------------
    const int c = (int)((L + 63u) >> 6), pad = 64 * c - (int)L;
    unsigned reg = 0;
    for (int k = 0; k < c; ++k) {
        const int idx = lane * c + k - pad;
        unsigned byte = 0;
        if (idx >= 0) byte = idx < 4 ? out8[idx] ^ 255u : out8[idx];
        reg = s_crc[(reg ^ byte) & 255u] ^ (reg >> 8);
    }
    unsigned g = 0x80000000u, sq = 0x00800000u;            // g = x^(8 c): square and multiply
    for (int e = c; e; e >>= 1) {
        if (e & 1) g = png_gfmul(g, sq);
        sq = png_gfmul(sq, sq);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned other = __shfl_xor(reg, d);
        reg = (lane & d) ? png_gfmul(other, g) ^ reg : png_gfmul(reg, g) ^ other;
        g = png_gfmul(g, g);
    }

    unsigned* slot = reinterpret_cast<unsigned*>(J.slots + gidx * J.slot);
    for (int w = lane; w < (int)((L + 3u) >> 2); w += 64) slot[w] = s_out[w];
    if (lane == 0) {
        PngStripRec R;
        R.len = L; R.crc = reg; R.a = (unsigned)(ad_a % SGS_PNG_ADLER); R.b = (unsigned)(ad_b % SGS_PNG_ADLER);
        J.rec[gidx] = R;
    }
}

// The bytes strip i's chunk takes in the file, with what goes before a frame's first chunk and after its last.
__device__ __forceinline__ unsigned long long png_chunk_bytes(const PngJob& J, long long i) {
    const int st = (int)(i % J.n_strips);
    return (unsigned long long)J.rec[i].len + 8ull + (st == 0 ? (unsigned long long)SGS_PNG_HEAD : 0ull) + (st == J.n_strips - 1 ? 9ull + 12ull : 0ull);
}

// place_files over the chunk sizes of every strip of every frame; the Adler-32 of each frame's filtered stream from its strips' sums.
__global__ __launch_bounds__(SGS_PNG_SCAN_THREADS) void k_png_scan(PngJob J) {
    __shared__ unsigned long long s_part[SGS_PNG_SCAN_THREADS];
    place_files<SGS_PNG_SCAN_THREADS>(J.sink, (long long)J.n_frames * J.n_strips, s_part, [&J](long long i) { return png_chunk_bytes(J, i); });
    // Adler-32 over N bytes f: a = 1 + sum f[i], b = N + sum (N - i) f[i]; a strip ending at byte `end` adds b_s + (N - end) a_s to b
    const long long rowlen = (long long)J.row_bytes + 1, N = rowlen * J.height;
    for (int f = (int)threadIdx.x; f < J.n_frames; f += SGS_PNG_SCAN_THREADS) {
        unsigned long long a = 1, b = (unsigned long long)(N % SGS_PNG_ADLER);
        long long end = 0;
        for (int s = 0; s < J.n_strips; ++s) {
            const int rows = min(J.rows_per_strip, J.height - s * J.rows_per_strip);
            end += rows * rowlen;
            const PngStripRec R = J.rec[(long long)f * J.n_strips + s];
            a = (a + R.a) % SGS_PNG_ADLER;
            b = (b + R.b + (unsigned long long)((N - end) % SGS_PNG_ADLER) * R.a) % SGS_PNG_ADLER;
        }
        J.adler[f] = (unsigned)(b << 16) | (unsigned)a;
    }
}

__device__ __forceinline__ void png_be32(unsigned char* p, unsigned v) {
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

// One workgroup per strip: the chunk, where the scan put it.  A frame whose end lies beyond the capacity is not written at all.
__global__ __launch_bounds__(SGS_PNG_GATHER_THREADS) void k_png_gather(PngJob J) {
    const int t = (int)threadIdx.x;
    const long long gidx = (long long)blockIdx.x;
    const int frame = (int)(gidx / J.n_strips), st = (int)(gidx % J.n_strips);
    long long at;
    if (!file_unit_offset(J.sink, gidx, J.n_strips, t == 0, at)) return;
    unsigned char* dst = J.sink.out + at;
    if (st == 0) {
        if (t < SGS_PNG_HEAD) dst[t] = J.head[t];
        dst += SGS_PNG_HEAD;
    }
    const PngStripRec R = J.rec[gidx];
    const bool last = st == J.n_strips - 1;
    const unsigned char* slot = J.slots + gidx * J.slot;
    for (unsigned i = (unsigned)t; i < R.len; i += SGS_PNG_GATHER_THREADS) dst[4 + i] = slot[i];
    if (t == 0) {
        png_be32(dst, R.len - 4u + (last ? 9u : 0u));
        unsigned char* p = dst + 4 + R.len;
        unsigned reg = R.crc;
        if (last) {                                        // the final block (stored, empty, BFINAL = 1) and the Adler-32 end the zlib stream
            p[0] = 1; p[1] = 0; p[2] = 0; p[3] = 0xFF; p[4] = 0xFF;
            png_be32(p + 5, J.adler[frame]);
            for (int k = 0; k < 9; ++k) {
                reg ^= p[k];
                for (int b = 0; b < 8; ++b) reg = (reg & 1u) ? (reg >> 1) ^ SGS_PNG_POLY : reg >> 1;
            }
            p += 9;
        }
        png_be32(p, ~reg);
        if (last) {
            const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
            for (int k = 0; k < 12; ++k) p[4 + k] = iend[k];
        }
    }
}

// ---- host side: the signature and the IHDR chunk -------------------------------------------------------------------------------------
namespace png {

inline unsigned crc32(const unsigned char* p, int n) {
    unsigned reg = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int b = 0; b < 8; ++b) reg = (reg & 1u) ? (reg >> 1) ^ SGS_PNG_POLY : reg >> 1;
    }
    return ~reg;
}

inline void build_head(unsigned char* h, int width, int height, bool depth16) {
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) h[i] = sig[i];
    unsigned char* c = h + 8;
    c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 13; c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
    for (int i = 0; i < 4; ++i) { c[8 + i] = (unsigned char)((unsigned)width >> (24 - 8 * i)); c[12 + i] = (unsigned char)((unsigned)height >> (24 - 8 * i)); }
    c[16] = depth16 ? 16 : 8;                              // bit depth
    c[17] = depth16 ? 0 : 2;                               // colour type: grey / RGB
    c[18] = 0; c[19] = 0; c[20] = 0;                       // deflate, adaptive filtering, no interlace
    const unsigned crc = crc32(c + 4, 17);
    for (int i = 0; i < 4; ++i) c[21 + i] = (unsigned char)(crc >> (24 - 8 * i));
}

}  // namespace png
}  // namespace sgs
