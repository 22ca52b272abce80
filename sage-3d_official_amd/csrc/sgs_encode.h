// sgs_encode.h — the device side of what the file encoders share (sgs_jpeg.h, sgs_png.h; DESIGN.md §11 "Placement"): how n
// variable-length units per frame (restart intervals, IDAT chunks) become files laid end to end in the caller's `out`.  A frame whose
// end lies beyond the capacity is not written at all, while its offset and size are still reported: one call tells what capacity the
// batch takes.  The host side (the pinned status words, the offsets array, the argument checks) is sgs_api.hip's FileScratch.
#pragma once

namespace sgs {

struct FileSink {
    long long* offs;                       // [units of the call + 1] where each unit starts in out (a frame's first unit: its file)
    unsigned char* out;
    long long cap;
    long long* out_offsets;
    long long* out_sizes;
    long long* status;                     // [0] bytes all files take, [1] the capacity they were given
};

// One workgroup of THREADS: offs[0..n] = the exclusive scan of bytes_of(i) over the n units of the call, and the status words.
// s_part: the caller's __shared__ [THREADS].
template <int THREADS, class BytesOf>
__device__ __forceinline__ void place_files(const FileSink& K, long long n, unsigned long long* s_part, BytesOf bytes_of) {
    const long long per = (n + THREADS - 1) / THREADS;
    const long long t0 = per * (long long)threadIdx.x, i0 = t0 < n ? t0 : n, i1 = i0 + per < n ? i0 + per : n;
    unsigned long long sum = 0;
    for (long long i = i0; i < i1; ++i) sum += bytes_of(i);
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < THREADS; ++t) { const unsigned long long v = s_part[t]; s_part[t] = run; run += v; }
        K.offs[n] = (long long)run;
        K.status[0] = (long long)run;
        K.status[1] = K.cap;
    }
    __syncthreads();
    unsigned long long at = s_part[threadIdx.x];
    for (long long i = i0; i < i1; ++i) {
        K.offs[i] = (long long)at;
        at += bytes_of(i);
    }
}

// A writer's first step, for unit `unit` of the call (frames of `per_frame` units each): reports the frame's offset and size (the
// `reporter` thread of the frame's first unit) and tells whether the frame fits the capacity; if it does, `at` is where the unit starts
// in out.
__device__ __forceinline__ bool file_unit_offset(const FileSink& K, long long unit, int per_frame, bool reporter, long long& at) {
    const int frame = (int)(unit / per_frame);
    const long long f0 = K.offs[(long long)frame * per_frame], f1 = K.offs[(long long)(frame + 1) * per_frame];
    if ((int)(unit % per_frame) == 0 && reporter) { K.out_offsets[frame] = f0; K.out_sizes[frame] = f1 - f0; }
    if (f1 > K.cap) return false;          // the frame does not fit: none of it is written
    at = K.offs[unit];
    return true;
}

}  // namespace sgs
