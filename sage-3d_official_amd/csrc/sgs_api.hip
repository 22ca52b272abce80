// sgs_api.hip — host side of libsage_gs.so: the C ABI of include/sage_gs.h over the gfx950 kernels.
//
// A frame is five stream-ordered launches (k_preprocess, k_bin_count, k_tile_scan, k_bin_emit, k_tile_render) with
// no host synchronisation in between (grids that depend on device-side counts are fixed-size and grid-stride); the
// frame's FrameStatus is copied to pinned host memory at the end and inspected when the caller synchronises.
// Ordinary frames run on the caller's stream with lane 0's intermediates; pipelined frames (SGS_FLAG_PIPELINED,
// sgs_render_batch) rotate over a few lanes, each with its own stream and intermediates, so that independent
// frames overlap on the chip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sage_gs.h"
#include "sgs_kernels.h"
#include "sgs_mesh.h"
#include "sgs_jpeg.h"
#include "sgs_png.h"
#include "sgs_resize.h"
#include "sgs_objects.h"
#include "sgs_similarity.h"
#include "sgs_topdown.h"
#include "sgs_clearance.h"
#include "sgs_geodesic.h"
#include "sgs_regions.h"
#include "sgs_endpoints.h"
#include "sgs_own.h"

namespace {

constexpr int kStatusRing = 256;
thread_local std::string g_create_error;

}  // namespace

using sgs::DevBuf;
using sgs::PinnedBuf;
using sgs::Grow;

// One Gaussian of a scene's PROBE (fine_shift_of): mean, 3-D covariance (+ its trace), ln(opacity), sampling weight — 512 of them, drawn at
// upload (layout_scene) and kept on the host.  Half of the draws are uniform over the scene, half proportional to the Gaussian's squared size
// (trace of its covariance): the record count of a scene with trained-3DGS statistics is carried by a few per cent of large splats, which a
// uniform sample of 512 holds a handful of — the estimate of the growth under a split was off by 20 % on such scenes and decided wrongly for
// one pose in six (r06w); with the mixture (each draw weighted by the inverse of its probability) the estimate follows the frame's real ratio.
struct ProbeSample { float m[3]; float S[6]; float ln_o; float trace; float wgt; };

struct sgs_scene {
    std::vector<ProbeSample> probe;     // (empty: fewer Gaussians than a probe is worth)
    int64_t n = 0, n_chunks = 0;
    int sh_degree = 0, sh_rows = 0;     // sh_rows: 16-byte rows of SH per Gaussian (12 at degree 3; 4 when sh_packed)
    bool sh_packed = false;             // uploaded from the compressed payload: the 8-bit coefficients stay bytes in HBM (k_scene_layout<true>)
    int sh_decode = 0;                  // ... and are read as sage_gs.h SGS_SH_DECODE_* says
    DevBuf<float4> geom, shq;
    DevBuf<float4> cbound;              // per chunk: bounding sphere of the means + largest scale (k_chunk_bounds)
    std::vector<unsigned> perm_host;    // Z-order: layout position -> original index (empty = identity)
    DevBuf<unsigned> inv;               // its inverse on the device: original index -> layout position (empty = identity); a frame's splat
                                        // records lie at layout positions and are found through it (sgs_kernels.h splat_at)
};

// The intermediates of ONE frame in flight.  Lane 0 serves ordinary frames on the caller's stream; pipelined
// frames (SGS_FLAG_PIPELINED, sgs_render_batch) rotate over all lanes, each on its own stream, so that a
// few frames overlap: binning is latency- and imbalance-bound, the composite issue-bound, and together they
// fill the chip better than back to back (measured +35 % frames/s with three lanes).
struct Lane {
    // per-Gaussian scratch (ensure_splats)
    DevBuf<Splat> splats;                        // one record per Gaussian, at its LAYOUT position (sgs_scene::inv)
    DevBuf<unsigned long long> vismask;          // per 64-Gaussian chunk: which slots are live this frame
    DevBuf<unsigned long long> bigmask;          //   ... and which of those went to the big-rect list
    DevBuf<unsigned> big_list;
    DevBuf<uint4> binrec;                        // per slot: depth bits, rect01, rect23 (dense copy for the binning kernels)
    DevBuf<unsigned> live_list;                  // chunks that passed the per-chunk bounds this frame (k_chunk_cull)
    // per-tile scratch (ensure_tiles)
    DevBuf<unsigned> tile_count, tile_offset;
    DevBuf<uint4> tile_order;                    // render order: (tile, first record, queue length) per position
    DevBuf<unsigned long long> tile_prof;        // profiling build: 8 words per tile
    DevBuf<unsigned long long> bin_prof;         // profiling build: 8 words per binning workgroup
    // binning scratch: per-workgroup (tile, base) lists
    DevBuf<uint2> blk_list;                      // per level-1 binning workgroup: (super-tile, base) of the super-tiles it touched
    DevBuf<unsigned> blk_len;
    // two-level binning: super-tile sub-counters / offsets (SGS_WT super-tiles at most), the level-2 job table and the jobs' bases
    DevBuf<unsigned> stile_count, stile_offset;
    DevBuf<uint4> jobs;
    DevBuf<unsigned> job_base;
    // per-record scratch (ensure_records): rec.cap is the lane's record capacity
    DevBuf<unsigned long long> rec;              // tile queues of (depth bits << 32 | slot) records
    DevBuf<unsigned long long> alt, part;        // scratch of the HBM radix path (oversized depth buckets only)
    DevBuf<unsigned> sorted_out;                 // SGS_FLAG_FULL_SORT (tests): fully ordered queues
    // pipelined frames
    sgs::Stream stream;                      // internal, non-blocking
    sgs::Event fork, done;
    bool busy = false;                       // has pipelined work that no synchronisation has collected yet
};

constexpr int kMaxLanes = 16;
constexpr int64_t kMaxRecords = 0xfffffff0ll;   // record capacity: tile offsets are 32-bit

// The collision-mesh depth path's own scratch (sgs_render_mesh_depth*): nothing of it is shared with the splat path's lanes.
struct MeshScratch {
    DevBuf<float4> rec;                      // the setup records: four rows per (triangle, frame) slot
    DevBuf<uint2> rect;                      //   ... and a rectangle and a big-list entry per slot
    DevBuf<unsigned> big;
    DevBuf<unsigned> counts, offs;           // per-tile counters / offsets of a group
    DevBuf<unsigned> list;                   // the record buffer: triangle ids of the per-tile lists
    int64_t cap_wanted = 4ll << 20;          // sgs_mesh_set_record_capacity (4 Mi records, 16 MiB)
    DevBuf<sgs::MeshStatus> d_st;            // [SGS_MESH_MAX_GROUP] + the upload check's word (ensure_mesh_status)
    PinnedBuf<sgs::MeshStatus> h_st;
    sgs::Event ev[2];
};

// What every file encoder keeps for the placement of its files (csrc/sgs_encode.h): an offset per unit and the pinned status words.
struct FileScratch {
    PinnedBuf<long long> h_status;           // [0] bytes needed, [1] capacity given, of the most recent call
    DevBuf<long long> offs;
};

// The JPEG encoder's scratch (sgs_encode_jpeg): per-interval lengths, the tables of the parameter sets seen so far (a table is never
// rewritten: an encode still in flight on another stream keeps reading its own) and the files' placement.
struct JpegScratch {
    struct Entry { int width, height, quality, s420; DevBuf<sgs::JpegTables> dev; };
    std::vector<Entry> tables;
    DevBuf<unsigned> sizes;
    FileScratch files;
};

// The PNG encoder's scratch (sgs_encode_png): a stored-size slot and a record per strip, an Adler-32 per frame, the files' placement.
struct PngScratch {
    DevBuf<sgs::PngStripRec> rec;
    DevBuf<unsigned char> slots;
    DevBuf<unsigned> adler;
    FileScratch files;
};

// The resize's scratch (sgs_resize): the horizontally resized frames of a call that runs both passes, and the tap tables of the axes
// seen so far (a table is never rewritten: a resize still in flight keeps reading its own).
struct ResizeScratch {
    struct Entry { int in, out, filter, format, ksize; DevBuf<int> bounds; DevBuf<unsigned char> weights; };
    std::vector<Entry> tables;
    DevBuf<unsigned> mid;
};

struct sgs_mesh {
    int64_t n_verts = 0, n_tris = 0;
    DevBuf<float> verts;
    DevBuf<int> tris;
    DevBuf<int> labels;                      // sgs_mesh_set_labels: [n_tris], or empty: a triangle's label is its index
};

// A frame's band, decided once per call by validate(): the 16-pixel tile rows [row_begin, row_end) the call owns (clamped), row k of them
// being row k * stride + phase of the frame (sgs_config.tile_row_stride / _phase), the frame's fine-tile shift z (fine_shift_of) and
// the pixel rows the call writes (band_pixel_rows).
struct Band {
    int row_begin = 0, row_end = 0, stride = 1, phase = 0, z = 0;
    int64_t pixel_rows = 0;
};

// One issued frame: where its verdict lands and its intermediates live, and what the statistics and sgs_debug_read need of it.
struct FrameRec {
    int slot = -1, lane = 0;                 // status ring slot (-1: no frame yet); the lane whose intermediates it used
    hipStream_t stream = nullptr;            // the caller's
    bool timed = false;
    int retries = 0;                         // renders it took beyond the first (synchronous frames grow the record buffers and render again)
    const sgs_scene* scene = nullptr;        // (nulled by sgs_scene_free)
    int64_t n = 0, pixels = 0;               // Gaussians; pixels the call wrote
    int sh_rows = 0;
    int T = 0, t_lo = 0, t_hi = 0, tiles = 0;    // the grid: all its tiles, the band [t_lo, t_hi) rendered (k_tile_scan fills only those), their count
};

// The status ring: a FrameStatus per frame in flight on the device, its pinned copy, and which slots are PENDING — issued since the
// last synchronisation and not looked at yet.  INVARIANT: a slot is pending only once the copy of its status word has been enqueued
// (issued() follows a successful enqueue; a slot whose enqueue failed was never taken).  The indices are nobody else's business.
class StatusRing {
    int next = 0, count = 0;                 // the pending slots: the `count` before `next` (mod kStatusRing)
public:
    DevBuf<FrameStatus> d_status;
    PinnedBuf<FrameStatus> h_status;
    std::unique_ptr<sgs::Event[]> ev;        // per-slot event sets for SGS_FLAG_TIMING, [kStatusRing][SGS_NUM_STAGES + 1] (ensure_timing_events)
    bool timed[kStatusRing] = {};            // the slot's frame recorded its events

    const sgs::Event* events(int slot) const { return &ev[(size_t)slot * (SGS_NUM_STAGES + 1)]; }
    bool full() const { return count == kStatusRing; }
    bool idle() const { return count == 0; }
    int slot() const { return next; }                                    // the slot of the next single frame (while !full()) ...
    void issued() { next = (next + 1) % kStatusRing; ++count; }         // ... pending from here on
    template <class F> void for_pending(F&& f) const { for (int k = count; k > 0; --k) f((next - k + kStatusRing) % kStatusRing); }
    void seen() { count = 0; }                                           // every pending verdict has been looked at
    // A batch chunk uses slots [0, cn) from the slot returned: cleared, copied back and read by the batch itself, hence never pending
    // (nothing else may be); the ring starts over.
    int take_chunk() { next = count = 0; return 0; }
};

struct sgs_ctx {
    int device = 0;
    MeshScratch mesh;
    JpegScratch jpeg;
    PngScratch png;
    ResizeScratch resize;
    std::string err;
    Lane lanes[kMaxLanes];
    int n_lanes = 3, next_lane = 0;          // sgs_tuning.lanes: lanes that SGS_FLAG_PIPELINED single frames rotate over
    int group = 8, group_lanes = 2;          // sgs_tuning.group x .group_lanes <= kMaxLanes: sgs_render_batch* issues `group` frames per
                                             // set of launches (blockIdx.y = frame), groups rotating over `group_lanes` streams
    int exp_grid = SGS_EXP_GRID;             // level-2 binning workgroups per launch (settled by A/B: r03, r04)
    int bin_grid = SGS_BIN_BLOCKS;           // binning workgroups per launch (<= SGS_BIN_BLOCKS)
    int pre_grid = 8192;                     // k_preprocess workgroups per launch of a frame GROUP: its waves loop over the live list (r03y)
    int64_t fine_tile_pixels = 640 * 480;    // sgs_tuning.fine_tile_pixels: frames of at most this many pixels may be rendered through 8x8-pixel
                                             // tiles (fine_shift_of; sgs_common.h "Fine tiles"); 0 = never
    double fine_tile_growth = 2.2;           // sgs_tuning.fine_tile_growth: ... while a split multiplies the frame's records by no more than this
    bool morton = true;                      // Z-order the scene at upload (sgs_tuning.morton = 0 keeps the caller's order): a chunk of 64
                                             // Gaussians is then a compact patch, which is what makes the per-chunk bounds
                                             // (k_chunk_bounds / chunk_outside) worth testing — trained scenes come in no spatial order
    DevBuf<unsigned long long> row_acc;      // records queued per frame tile row, summed over the frames since the last
                                             // sgs_row_records(reset) — what cost-balanced tile-row bands are cut from
    int64_t rec_cap_wanted = 16ll << 20;
    StatusRing ring;
    FrameRec last;                           // the most recent frame issued: what sgs_frame_sync reports and sgs_debug_read looks at
};

#define SGS_FAIL(ctx, code, ...)                                  \
    do {                                                          \
        char buf_[512];                                           \
        snprintf(buf_, sizeof buf_, __VA_ARGS__);                 \
        (ctx)->err = buf_;                                        \
        return (code);                                            \
    } while (0)

#define SGS_HIP(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            SGS_FAIL(ctx, e_ == hipErrorOutOfMemory ? SGS_ERR_OOM : SGS_ERR_HIP, "%s: %s", #call, \
                     hipGetErrorString(e_));                                                   \
    } while (0)

#define SGS_TRY(check) do { if (const int rc_ = (check)) return rc_; } while (0)

namespace {

// The argument checks of the operator entry points (sgs_resize .. sgs_geodesic_path): each is SGS_OK, or the context's message and
// SGS_ERR_INVALID.  An entry point lists them in the order it refuses in; what these cannot say is a plain SGS_FAIL beside them.
// non_null and aligned take any number of (pointer, name) pairs and judge them in the order given.  The object table, the top-down
// map and the clearance map spell their alignment tests out: tests/test_emu_*_mutants.py take those lines out by their text.
struct Args {
    sgs_ctx* ctx;
    const char* who;
    int non_null() const { return SGS_OK; }
    template <class... More>
    int non_null(const void* p, const char* name, More... more) const {
        if (!p) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: null %s", who, name);
        return non_null(more...);
    }
    int aligned(int) const { return SGS_OK; }
    template <class... More>
    int aligned(int bytes, const void* p, const char* name, More... more) const {          // (a null pointer is aligned: whether it may be null is non_null's to say)
        if (reinterpret_cast<uintptr_t>(p) % bytes) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %s %p is not %d-byte aligned", who, name, p, bytes);
        return aligned(bytes, more...);
    }
    // Frames (maps) a stride apart, of `need` elements each, do not overlap.  `text` is the entry point's own wording of the refusal
    // after "<who>: ", with two %lld: the stride and `need`.
    int frames_fit(int64_t stride, int64_t need, const char* text) const {
        if (stride < need) SGS_FAIL(ctx, SGS_ERR_INVALID, (std::string("%s: ") + text).c_str(), who, (long long)stride, (long long)need);
        return SGS_OK;
    }
    // The byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte.
    static bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
        const uint64_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
        return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
    }
    int disjoint(const void* a, uint64_t a_bytes, const char* a_name, const void* b, uint64_t b_bytes, const char* b_name) const {
        if (overlap(a, a_bytes, b, b_bytes)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %s %p and %s %p overlap", who, a_name, a, b_name, b);
        return SGS_OK;
    }
    int grid_within(int nx, int ny, int max) const {
        if (nx < 1 || ny < 1 || nx > max || ny > max) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: nx = %d, ny = %d (1 <= nx, ny <= %d)", who, nx, ny, max);
        return SGS_OK;
    }
};

// f(first, count) for each run of at most `max` of n frames (maps, words): what one launch takes in gridDim.y or in its arguments.
template <class F>
void for_chunks(int n, int max, F f) {
    for (int first = 0; first < n; first += max) f(first, std::min(max, n - first));
}

// A counter array that the kernels keep zeroed from then on needs ONE clear, at its allocation.  hipMemset of device memory runs on the
// NULL stream and may return before it has run; the frames use non-blocking streams that do not order with it — an unfinished clear would
// land in the middle of a frame's counting — hence the synchronisation.  An array that could not be cleared is not kept.
template <class T>
int grow_zeroed(sgs_ctx* ctx, DevBuf<T>& b, int64_t want) {
    if (b.holds(want)) return SGS_OK;
    SGS_HIP(ctx, b.grow(want));
    hipError_t e = hipMemset(b.p, 0, (size_t)want * sizeof(T));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { b.reset(); SGS_FAIL(ctx, SGS_ERR_HIP, "clearing a counter array: %s", hipGetErrorString(e)); }
    return SGS_OK;
}

// The ensure_* functions: every array of a set present at the capacity the frame needs.  Each growth decides by its own array (one
// comparison when it is large enough), so an allocation that failed half-way through a set is simply made again by the next frame.
int ensure_splats(sgs_ctx* ctx, Lane& L, int64_t n) {
    const int64_t chunks = std::max<int64_t>(1, (n + 63) / 64);
    const int64_t cap = chunks * 64;
    int rc;
    SGS_HIP(ctx, L.splats.grow(cap));
    SGS_HIP(ctx, L.vismask.grow(chunks));
    SGS_HIP(ctx, L.bigmask.grow(chunks));
    SGS_HIP(ctx, L.binrec.grow(cap));
    SGS_HIP(ctx, L.live_list.grow(chunks * (1 + SGS_MAX_GROUP) + 2));       // the list | a group's work list (sgs_work_list)
    SGS_HIP(ctx, L.big_list.grow(SGS_BIG_CAP));
    SGS_HIP(ctx, L.blk_len.grow(SGS_BIN_BLOCKS * 2));                       // list lengths | XCD ids
    SGS_HIP(ctx, L.blk_list.grow((int64_t)SGS_BIN_BLOCKS * SGS_WT));
    // k_bin_emit zeroes every count k_stile_scan has consumed
    if ((rc = grow_zeroed(ctx, L.stile_count, (int64_t)SGS_WT * SGS_XCDS)) != SGS_OK) return rc;
    SGS_HIP(ctx, L.stile_offset.grow((int64_t)SGS_WT * SGS_XCDS + 1));
    SGS_HIP(ctx, L.bin_prof.grow(SGS_BIN_BLOCKS * 8));
    return SGS_OK;
}

int ensure_tiles(sgs_ctx* ctx, Lane& L, int tiles) {
    int rc;
    // level 2: one counter per tile; k_expand<true> zeroes every count k_tile_scan has consumed
    if ((rc = grow_zeroed(ctx, L.tile_count, (int64_t)tiles + 1)) != SGS_OK) return rc;
    SGS_HIP(ctx, L.tile_offset.grow((int64_t)tiles + 1));
    SGS_HIP(ctx, L.tile_prof.grow((int64_t)tiles * SGS_PROF_WORDS));
    SGS_HIP(ctx, L.tile_order.grow(tiles));
    return SGS_OK;
}

// The record arrays of a lane share ONE capacity, rec.cap (what the kernels are told: fill_params), or are all empty.
void release_records(Lane& L) { L.rec.reset(); L.alt.reset(); L.part.reset(); L.jobs.reset(); L.job_base.reset(); }

int grow_records(sgs_ctx* ctx, Lane& L, int64_t cap) {
    SGS_HIP(ctx, L.rec.grow(cap));
    SGS_HIP(ctx, L.alt.grow(cap));
    SGS_HIP(ctx, L.part.grow(cap));
    // level-2 jobs: the super-tile queues (cap / 2 records of 16 bytes, in `alt`) in segments of SGS_SEG, plus one ragged
    // segment per super-tile
    const int64_t jcap = cap / 2 / SGS_SEG + SGS_WT + 1;
    SGS_HIP(ctx, L.jobs.grow(jcap));
    SGS_HIP(ctx, L.job_base.grow(jcap * (SGS_ST * SGS_ST)));
    return SGS_OK;
}

// ... at exactly the capacity wanted: sgs_set_record_capacity empties every lane's, growth does the rest.
int ensure_records(sgs_ctx* ctx, Lane& L) {
    const int64_t cap = std::max<int64_t>(ctx->rec_cap_wanted, 1024);
    if (cap > kMaxRecords) SGS_FAIL(ctx, SGS_ERR_INVALID, "record capacity %lld exceeds 2^32", (long long)cap);
    const int rc = grow_records(ctx, L, cap);
    if (rc != SGS_OK) release_records(L);
    return rc;
}

int ensure_sorted_out(sgs_ctx* ctx, Lane& L) {
    SGS_HIP(ctx, L.sorted_out.grow(L.rec.cap));
    return SGS_OK;
}

// A lane's stream and events exist from its first pipelined frame on.
int ensure_lane_stream(sgs_ctx* ctx, Lane& L) {
    SGS_HIP(ctx, L.stream.create(hipStreamNonBlocking));
    SGS_HIP(ctx, L.fork.create(hipEventDisableTiming));
    SGS_HIP(ctx, L.done.create(hipEventDisableTiming));
    return SGS_OK;
}

// The event sets of SGS_FLAG_TIMING: all of them or none.
int ensure_timing_events(sgs_ctx* ctx) {
    if (ctx->ring.ev) return SGS_OK;
    constexpr int n = kStatusRing * (SGS_NUM_STAGES + 1);
    std::unique_ptr<sgs::Event[]> ev(new (std::nothrow) sgs::Event[n]);
    if (!ev) SGS_FAIL(ctx, SGS_ERR_OOM, "out of host memory");
    for (int i = 0; i < n; ++i) SGS_HIP(ctx, ev[i].create());
    ctx->ring.ev = std::move(ev);
    return SGS_OK;
}

// The mesh path's status words, on the device and pinned: made by the first mesh upload or mesh frame of a context.
int ensure_mesh_status(sgs_ctx* ctx) {
    SGS_HIP(ctx, ctx->mesh.d_st.grow(SGS_MESH_MAX_GROUP + 1));
    SGS_HIP(ctx, ctx->mesh.h_st.grow(SGS_MESH_MAX_GROUP + 1));
    return SGS_OK;
}

// Host-wait for every pipelined frame in flight.
int drain_lanes(sgs_ctx* ctx) {
    for (int l = 0; l < kMaxLanes; ++l) {
        Lane& L = ctx->lanes[l];
        if (L.busy) { SGS_HIP(ctx, hipEventSynchronize(L.done.e)); L.busy = false; }
    }
    return SGS_OK;
}

// Fine tiles (sgs_common.h): the shift z of a call — its frame is rendered through tiles of (16 >> z)^2 pixels.  A function of the scene, the
// camera and the configuration ALONE, so that a frame is the same frame however it is issued (alone, pipelined, in a batch, as a band).
//   * Never under the test hooks whose point is the REFERENCE's integer structures — queues and offsets of 16x16-pixel tiles.
//   * Small frames only: z <= the number of times the frame's pixel count, quadrupled, stays within sgs_tuning.fine_tile_pixels (640x480
//     -> 1, 320x240 -> 2) — a large frame fills the chip with 16x16 tiles.
//   * And only while halving the tiles does not multiply the RECORDS by more than sgs_tuning.fine_tile_growth (2.2).  Every record is binned, partitioned, ranked and
//     quadrant-tested once per tile it lands in, so what a split costs is the growth of D — small where splats are smaller than the tiles
//     (x1.5-2.0 on the indoor scenes: the split wins 20-50 % of a frame), towards x4 where they are larger (x2.5-3.5 on scenes with
//     trained-3DGS statistics, whose pixels saturate inside the first batch anyway: there the split LOSES 30 %).  Measured per pose, both
//     scene kinds, three resolutions (profiles/r06w_fine_tiles_growth_rule.txt): the frame's time is shorter with the split below a growth of
//     2.1-2.4 and longer above; the rule lands within 1 % of choosing the better tiling per pose.  D at each tile size is ESTIMATED here, on
//     the host, from the scene's probe — a thousand Gaussians projected with S2's arithmetic (fp32) and binned over the extent of
//     {alpha >= alpha_min} as k_preprocess bins it: ~10 us per frame, within a few per cent of the frame's real D ratio.
// floor / ceil of a value well inside the int range, without the libm call a portable build makes of std::floor
inline int ifloor(float v) { const int i = (int)v; return i - (v < (float)i ? 1 : 0); }
inline int iceil(float v) { const int i = (int)v; return i + (v > (float)i ? 1 : 0); }
int fine_shift_of(const sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config& cfg) {
    if (cfg.flags & (SGS_FLAG_NO_FINE_TILES | SGS_FLAG_FULL_SORT | SGS_FLAG_LOOSE_CULL)) return 0;
    int zcap = 0;
    while (zcap < 2 && (((int64_t)cam->width * cam->height) << (2 * zcap)) <= ctx->fine_tile_pixels) ++zcap;
    if (zcap == 0 || !scene || scene->probe.empty() || ctx->fine_tile_growth >= 16.0) return zcap;
    const float* V = cam->view;
    const float fx = cam->fx, fy = cam->fy, W = (float)cam->width, H = (float)cam->height;
    const float limx = cfg.clamp * (0.5f * W / fx), limy = cfg.clamp * (0.5f * H / fy);
    const float ln_amin = std::log(cfg.alpha_min);
    const float jb = std::max(fx, fy), jk = 2.0f + limx * limx + limy * limy;
    double D[3] = {0.0, 0.0, 0.0};
    for (const ProbeSample& g : scene->probe) {
        const float tz = V[8] * g.m[0] + V[9] * g.m[1] + V[10] * g.m[2] + V[11];
        if (!(tz > cfg.near_z) || !(tz <= cfg.far_z)) continue;
        const float K = 2.0f * (g.ln_o - ln_amin);                    // alpha >= alpha_min  <=>  d^T Sigma'^-1 d <= K
        if (!(K > 0.0f)) continue;                                    // (never blended: nothing is binned)
        const float tx = V[0] * g.m[0] + V[1] * g.m[1] + V[2] * g.m[2] + V[3], ty = V[4] * g.m[0] + V[5] * g.m[1] + V[6] * g.m[2] + V[7];
        const float itz = 1.0f / tz, xz = tx * itz, yz = ty * itz;
        const float px = fx * xz + cam->cx - 0.5f, py = fy * yz + cam->cy - 0.5f;
        {   // off screen by more than any footprint it can have (k_preprocess's own pre-check: lambda_max <= |J|_F^2 trace(Sigma) + dilation,
            // radius <= 3 sqrt(2 lambda_max + 0.3163) + 1, squared and rounded up): most of a probe ends here
            const float jf = jb * itz, lmax = jf * jf * jk * g.trace + cfg.dilation;
            const float rb2 = 9.5f * (2.0f * lmax + 0.3163f) + 4.0f;
            const float ox = px < 0.0f ? -px : px > W ? px - W : 0.0f, oy = py < 0.0f ? -py : py > H ? py - H : 0.0f;
            if (ox * ox > rb2 || oy * oy > rb2) continue;
        }
        const float txc = std::min(limx, std::max(-limx, xz)) * tz, tyc = std::min(limy, std::max(-limy, yz)) * tz;
        const float j00 = fx * itz, j02 = -fx * txc * itz * itz, j11 = fy * itz, j12 = -fy * tyc * itz * itz;
        const float T0[3] = {j00 * V[0] + j02 * V[8], j00 * V[1] + j02 * V[9], j00 * V[2] + j02 * V[10]};
        const float T1[3] = {j11 * V[4] + j12 * V[8], j11 * V[5] + j12 * V[9], j11 * V[6] + j12 * V[10]};
        const float* S = g.S;                                         // (00, 01, 02, 11, 12, 22)
        const float u0 = S[0] * T0[0] + S[1] * T0[1] + S[2] * T0[2], u1 = S[1] * T0[0] + S[3] * T0[1] + S[4] * T0[2], u2 = S[2] * T0[0] + S[4] * T0[1] + S[5] * T0[2];
        const float w0 = S[0] * T1[0] + S[1] * T1[1] + S[2] * T1[2], w1 = S[1] * T1[0] + S[3] * T1[1] + S[4] * T1[2], w2 = S[2] * T1[0] + S[4] * T1[1] + S[5] * T1[2];
        const float a = T0[0] * u0 + T0[1] * u1 + T0[2] * u2 + cfg.dilation, b = T1[0] * u0 + T1[1] * u1 + T1[2] * u2,
                    c = T1[0] * w0 + T1[1] * w1 + T1[2] * w2 + cfg.dilation;
        const float det = a * c - b * b;
        if (!(det > 0.0f)) continue;
        const float mid = 0.5f * (a + c), r3 = 3.0f * __builtin_sqrtf(mid + __builtin_sqrtf(std::max(0.1f, mid * mid - det)));     // S3
        if (!(r3 < 1.0e6f) || !(std::fabs(px) < 1.0e6f) || !(std::fabs(py) < 1.0e6f)) continue;       // (NaN / wild values: not a probe worth counting)
        const float radius = (float)iceil(r3);
        const float hx = std::min(__builtin_sqrtf(K * a), radius), hy = std::min(__builtin_sqrtf(K * c), radius);
        if (!(hx >= 0.0f) || !(hy >= 0.0f)) continue;
        const float xa = px - hx, xb = px + hx, ya = py - hy, yb = py + hy;
        float icp = 1.0f / SGS_TILE;
        for (int z = 0; z <= zcap; ++z, icp *= 2.0f) {                // cells of cp = 16 >> z pixels: a cell holds the pixel centres cp t .. cp t + cp - 1
            const int cp = SGS_TILE >> z, gxz = (cam->width + cp - 1) / cp, gyz = (cam->height + cp - 1) / cp;
            const int nx = std::min(gxz, ifloor(xb * icp) + 1) - std::max(0, iceil((xa - (float)(cp - 1)) * icp));
            const int ny = std::min(gyz, ifloor(yb * icp) + 1) - std::max(0, iceil((ya - (float)(cp - 1)) * icp));
            if (nx > 0 && ny > 0) D[z] += (double)g.wgt * (double)(nx * ny);
        }
    }
    int z = 0;
    while (z < zcap && D[z + 1] <= ctx->fine_tile_growth * D[z]) ++z;     // (nothing of the probe in view: 0 <= 0, the pixel rule alone)
    return z;
}

// What every path asks of a camera (sage_gs.h): nullptr, or what is wrong with it (in `why`).
const char* check_camera(const sgs_camera& cam, char* why, size_t n_why) {
    if (cam.width <= 0 || cam.height <= 0 || cam.width > 65535 * SGS_TILE || cam.height > 65535 * SGS_TILE) {
        snprintf(why, n_why, "bad resolution %dx%d", cam.width, cam.height); return why;
    }
    if (!(cam.fx > 0.f) || !(cam.fy > 0.f)) { snprintf(why, n_why, "focal lengths must be positive"); return why; }
    // the view must be rigid: k_preprocess's fp32 screen-bound exclusion prices a Gaussian's footprint with |J|_F^2 s_max^2, which a
    // scaled or sheared view would break silently (a USD xformOp:scale != 1 has to be applied to the Gaussians' means and scales by
    // the caller), and the mesh path's depth is the camera-space z of a rigid view
    const float* V = cam.view;
    for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) {
            const double d = (double)V[4 * r] * V[4 * c] + (double)V[4 * r + 1] * V[4 * c + 1] + (double)V[4 * r + 2] * V[4 * c + 2];
            // (fp32 pose matrices are orthonormal to ~1e-6; the per-chunk bounds and the footprint bound of k_preprocess
            //  absorb ~1e-4 of non-rigidity, so the contract is an order of magnitude inside that)
            if (!(std::fabs(d - (r == c ? 1.0 : 0.0)) < 1.0e-5)) {
                snprintf(why, n_why, "view is not rigid: rows %d.%d of its 3x3 give %g", r, c, d); return why;
            }
        }
    return nullptr;
}

// Pixel rows of a frame of `height` that the 16-pixel tile rows [row_begin, row_end) of a call cover, row k of the call being row
// k * stride + phase of the frame (sgs_config.tile_row_stride / _phase).  The same count under fine tiles: a 16-pixel row is 2^z rows
// of cells, clipped to the same height.
int64_t band_pixel_rows(int height, int row_begin, int row_end, int stride, int phase) {
    int64_t rows = 0;
    for (int k = row_begin; k < row_end; ++k) {
        const int y0 = (k * stride + phase) * SGS_TILE;
        rows += std::max(0, std::min(y0 + SGS_TILE, height) - y0);
    }
    return rows;
}

// The checks every frame passes before anything is enqueued, and the frame's band (rows as the caller gave them: negative = open end).
int validate(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config* cfg,
             int row_begin, int row_end, const float* out_rgb, Band& band) {
    if (!scene || !cam || !out_rgb) SGS_FAIL(ctx, SGS_ERR_INVALID, "null scene / camera / output");
    char why[160];
    if (check_camera(*cam, why, sizeof why)) SGS_FAIL(ctx, SGS_ERR_INVALID, "camera: %s", why);
    const int stride = cfg && cfg->tile_row_stride > 1 ? cfg->tile_row_stride : 1, phase = cfg && stride > 1 ? cfg->tile_row_phase : 0;
    if (phase < 0 || phase >= stride) SGS_FAIL(ctx, SGS_ERR_INVALID, "tile_row_phase %d outside [0, stride %d)", phase, stride);
    const int gy_frame = (cam->height + SGS_TILE - 1) / SGS_TILE;
    const int gy = gy_frame > phase ? (gy_frame - phase + stride - 1) / stride : 0;      // rows this call owns
    if (row_end < 0 || row_end > gy) row_end = gy;
    if (row_begin < 0) row_begin = 0;
    if (row_begin > row_end) SGS_FAIL(ctx, SGS_ERR_INVALID, "tile_row_begin %d > tile_row_end %d", row_begin, row_end);
    if (cfg && cfg->sh_degree > 3) SGS_FAIL(ctx, SGS_ERR_INVALID, "sh_degree %d > 3", cfg->sh_degree);
    if (cfg) {
        // what the kernels lean on: depth keys are the bits of a POSITIVE float >= near_z (unsigned order, the composite's
        // bucket index (key >> 18) - (bits(near_z) >> 18), 1 / tz), and the thresholds are compared as bit patterns
        if (!(cfg->near_z > 0.f) || !(cfg->far_z > cfg->near_z)) SGS_FAIL(ctx, SGS_ERR_INVALID, "need 0 < near_z < far_z (got %g, %g)", cfg->near_z, cfg->far_z);
        if (!(cfg->alpha_min > 0.f) || !(cfg->alpha_min < 1.f) || !(cfg->alpha_max >= cfg->alpha_min) || !(cfg->alpha_max < 1.f))
            SGS_FAIL(ctx, SGS_ERR_INVALID, "need 0 < alpha_min <= alpha_max < 1 (got %g, %g)", cfg->alpha_min, cfg->alpha_max);
        if (!(cfg->t_min > 0.f) || !(cfg->t_min < 1.f)) SGS_FAIL(ctx, SGS_ERR_INVALID, "need 0 < t_min < 1 (got %g)", cfg->t_min);
        if (!(cfg->dilation >= 0.f) || !(cfg->clamp > 0.f)) SGS_FAIL(ctx, SGS_ERR_INVALID, "need dilation >= 0 and clamp > 0");
    }
    if (gy_frame > SGS_MAX_ROWS) SGS_FAIL(ctx, SGS_ERR_INVALID, "height %d exceeds %d tile rows", cam->height, SGS_MAX_ROWS);
    // level 1 of the binning keeps one counter per super-tile of the band in LDS (the band's rows and tiles as the kernels count them:
    // cells of (16 >> z)^2 pixels, sgs_common.h "Fine tiles")
    sgs_config cfg_d;
    if (!cfg) sgs_config_default(&cfg_d);
    const int z = fine_shift_of(ctx, scene, cam, cfg ? *cfg : cfg_d), cp = SGS_TILE >> z;
    const int gx = (cam->width + cp - 1) / cp, rb = row_begin << z, re = row_end << z;
    const int64_t ns = (int64_t)((gx + SGS_ST - 1) / SGS_ST) * (((re + SGS_ST - 1) / SGS_ST) - rb / SGS_ST);
    if (ns > SGS_WT) SGS_FAIL(ctx, SGS_ERR_INVALID, "band of %d tile rows x %d tiles exceeds %d super-tiles", re - rb, gx, SGS_WT);
    band.row_begin = row_begin; band.row_end = row_end; band.stride = stride; band.phase = phase; band.z = z;
    band.pixel_rows = band_pixel_rows(cam->height, row_begin, row_end, stride, phase);
    return SGS_OK;
}

void fill_params(FrameParams& P, const sgs_ctx* ctx, const Lane& L, const sgs_scene* scene, const sgs_camera* cam,
                 const sgs_config& cfg, const Band& band) {
    memset(&P, 0, sizeof P);
    for (int i = 0; i < 12; ++i) P.view[i] = cam->view[i];
    const float* V = cam->view;
    for (int c = 0; c < 3; ++c)
        P.campos[c] = -((double)V[c] * V[3] + (double)V[4 + c] * V[7] + (double)V[8 + c] * V[11]);
    P.fx = cam->fx; P.fy = cam->fy; P.cx = cam->cx; P.cy = cam->cy;
    P.near_z = cfg.near_z; P.far_z = cfg.far_z; P.dilation = cfg.dilation; P.clamp = cfg.clamp;
    P.alpha_min = cfg.alpha_min; P.alpha_max = cfg.alpha_max; P.t_min = cfg.t_min;
    for (int c = 0; c < 3; ++c) P.bg[c] = cfg.bg[c];
    P.width = cam->width; P.height = cam->height;
    // Fine tiles (sgs_common.h): the grid, the band and every tile index the kernels see count CELLS of (16 >> z)^2 pixels; row_begin / row_end
    // arrive in 16-pixel rows (the C ABI's unit), each of which is 2^z rows of cells — but for the frame's last one when the height leaves it short
    const int row_begin = band.row_begin, row_end = band.row_end, z = band.z, cp = SGS_TILE >> z;
    const int gx16 = (cam->width + SGS_TILE - 1) / SGS_TILE, gy16 = (cam->height + SGS_TILE - 1) / SGS_TILE;
    P.gx = (cam->width + cp - 1) / cp; P.gy = (cam->height + cp - 1) / cp;
    P.row_stride = band.stride; P.row_phase = band.phase;
    P.row_begin = row_begin << z; P.row_end = row_end << z;
    if (row_end > row_begin && (row_end - 1) * P.row_stride + P.row_phase == gy16 - 1) P.row_end -= (gy16 << z) - P.gy;
    // a contiguous band ignores what projects outside its pixel rows; interleaved rows span the frame
    P.cull_y0 = P.row_stride > 1 ? 0 : SGS_TILE * row_begin;
    P.cull_y1 = P.row_stride > 1 ? SGS_TILE * gy16 : SGS_TILE * row_end;
    P.sh_degree = cfg.sh_degree < 0 ? scene->sh_degree : std::min(cfg.sh_degree, scene->sh_degree);
    P.sh_rows = scene->sh_rows;
    P.n = scene->n; P.n_chunks = scene->n_chunks;
    P.n_ranges = (int32_t)((scene->n + SGS_RANGE - 1) / SGS_RANGE);
    P.n_windows = 1;                                                              // (one window of super-tiles: sgs_kernels.h, level 1)
    P.limx = (double)P.clamp * (0.5 * (double)P.width / (double)P.fx); P.limy = (double)P.clamp * (0.5 * (double)P.height / (double)P.fy);
    P.rec_capacity = L.rec.cap;
    P.job_capacity = (int32_t)std::min<int64_t>(L.jobs.cap, 0x7fffffff);
    P.flags = (cfg.flags & ~SGS_PFLAG_INTERNAL) | (scene->sh_packed ? SGS_PFLAG_SH_PACKED | ((uint32_t)scene->sh_decode << SGS_PFLAG_SH_MODE_SHIFT) : 0u) |
              ((uint32_t)z << SGS_PFLAG_FINE_SHIFT);
    {   // k_chunk_cull's planes (sgs_kernels.h chunk_outside: the derivation and why each constant is conservative)
        const double lx = P.limx, ly = P.limy;
        P.cull_A = 1.001 * 3.0 * std::sqrt(2.0 * (2.0 + lx * lx + ly * ly)) * std::max((double)P.fx, (double)P.fy) * 1.0001;
        const double c0 = 1.001 * (3.0 * std::sqrt(2.0 * (double)P.dilation + 0.3163) + 1.0) + 0.5 + 1.0;      // + one pixel of slack
        P.cull_off[0] = (double)P.cx - 0.5 + c0;                                     // px + rb >= 0
        P.cull_off[1] = (double)(SGS_TILE * gx16) - (double)P.cx + 0.5 + c0;         // px - rb <  16 gx (gx: 16-pixel tiles)
        P.cull_off[2] = (double)P.cy - 0.5 - (double)P.cull_y0 + c0;                 // py + rb >= cull_y0
        P.cull_off[3] = (double)P.cull_y1 - (double)P.cy + 0.5 + c0;                 // py - rb <  cull_y1
        const double f[4] = {(double)P.fx, (double)P.fx, (double)P.fy, (double)P.fy};
        for (int k = 0; k < 4; ++k) P.cull_nrm[k] = std::sqrt(f[k] * f[k] + P.cull_off[k] * P.cull_off[k]);
    }
}

// ---- the launches of a frame (group), stage by stage.  G.s[0 .. nf) are the group's frames (same resolution and tile rows). ----
// S1-S3: per-chunk bounds -> the frame's live list, then the projection (k_chunk_cull, k_preprocess)
void launch_cull(const FrameGroup& G, int nf, hipStream_t stream, bool share = false) {
    const FrameParams& P = G.s[0].P;
    if (P.n_chunks > 0 && share)       // (the lists of all frames of the group + the group's work list, one lane per chunk)
        hipLaunchKernelGGL(sgs::k_chunk_cull_group, dim3((unsigned)((P.n_chunks + SGS_CULL_THREADS - 1) / SGS_CULL_THREADS)), dim3(SGS_CULL_THREADS), 0, stream,
                           G, (unsigned)nf);
    else if (P.n_chunks > 0)
        hipLaunchKernelGGL(sgs::k_chunk_cull, dim3((unsigned)((P.n_chunks + SGS_CULL_THREADS - 1) / SGS_CULL_THREADS), (unsigned)nf),
                           dim3(SGS_CULL_THREADS), 0, stream, G);
}
void launch_project(const sgs_ctx* ctx, const FrameGroup& G, int nf, hipStream_t stream) {
    const FrameParams& P = G.s[0].P;
    if (P.n_chunks <= 0) return;
    const bool fine = ((P.flags >> SGS_PFLAG_FINE_SHIFT) & 3u) != 0u;        // (fine tiles: the instantiation that scales the splats, sgs_common.h)
    const int64_t all = (P.n_chunks + 3) / 4, cap = std::max(256, ctx->pre_grid / nf);
    const bool narrow = nf > 1 && 2 * (P.row_end - P.row_begin) < P.gy && cap < all;
    // The full frames of a GROUP share what they read of the scene: one cull kernel writes every frame's live list and the group's work
    // list — (chunk, frame) pairs, chunk-major — and the projection's waves take THAT (k_preprocess_shared), so the frames that want a chunk
    // run side by side and its 15 KiB of rows come from HBM once.  Never slower than every frame walking its own list in its own part of
    // the grid, whatever the views share (profiles/r06zb: +-0 at an overlap of 1.3 of 4, -2 ... -5 % per frame at the bench's 1.4, -9 % at
    // 2.3, -7 ... -10 % for a trajectory's consecutive headings); frames bit-identical.  (SGS_NO_SHARE: A/B builds, scripts/build_variant.sh.)
#ifdef SGS_NO_SHARE
    const bool share = false;
#else
    const bool share = nf > 1 && !narrow;
#endif
    launch_cull(G, nf, stream, share);
    // a wave per chunk of the scene (most end at once) — except for a group of narrow bands, whose frames share
    // pre_grid workgroups that loop over the live list (r03y: 0.0454 -> 0.0425 ms per frame of a 3-row band)
    if (narrow) {
        if (fine) hipLaunchKernelGGL((sgs::k_preprocess<true, true>), dim3((unsigned)cap, (unsigned)nf), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_preprocess<true, false>), dim3((unsigned)cap, (unsigned)nf), dim3(256), 0, stream, G);
    } else if (share) {
        const unsigned grid = (unsigned)((all * nf + SGS_XCDS - 1) / SGS_XCDS + 1) * SGS_XCDS;       // (every XCD's eighth of the list, rounded up)
        if (fine) hipLaunchKernelGGL((sgs::k_preprocess_shared<true>), dim3(grid), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_preprocess_shared<false>), dim3(grid), dim3(256), 0, stream, G);
    } else {
        if (fine) hipLaunchKernelGGL((sgs::k_preprocess<false, true>), dim3((unsigned)all, (unsigned)nf), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_preprocess<false, false>), dim3((unsigned)all, (unsigned)nf), dim3(256), 0, stream, G);
    }
}
// S4, two levels (six launches); ev_mid (nullable) is recorded between the levels
int launch_binning(sgs_ctx* ctx, const FrameGroup& G, int nf, hipStream_t stream, hipEvent_t ev_mid) {
    const FrameParams& P = G.s[0].P;
    const unsigned F = (unsigned)nf;
    const int gx = P.gx, row_begin = P.row_begin, row_end = P.row_end;
    // the binning grids are sized per LAUNCH: the frames of a group share them (a group of four band frames with 512 + 2048
    // workgroups EACH spent its time starting workgroups that found a chunk or a job apiece: 0.047 -> 0.041 ms per frame
    // of a 3-row band, 0.057 -> 0.051 of an 18-row one, r03y)
    const unsigned bin_blocks = (unsigned)std::min<int64_t>(std::max(32, ctx->bin_grid / nf), P.n_ranges);
    // level 1: splats -> super-tile queues (count, scan + level-2 job list, emit)
    const int gxs = (gx + SGS_ST - 1) / SGS_ST, ns = gxs * ((row_end + SGS_ST - 1) / SGS_ST - row_begin / SGS_ST);
    const size_t win_bytes = (size_t)((std::max(ns, 1) + 127) / 128) * 128 * sizeof(unsigned);
    const bool bin = P.n_ranges > 0 && ns > 0;
    if (bin) hipLaunchKernelGGL(sgs::k_bin_count, dim3(bin_blocks, F), dim3(SGS_BIN_THREADS), win_bytes, stream, G);
    hipLaunchKernelGGL(sgs::k_stile_scan, dim3(1, F), dim3(SGS_SSCAN_THREADS), 0, stream, G);
    if (bin) hipLaunchKernelGGL(sgs::k_bin_emit, dim3(bin_blocks, F), dim3(SGS_BIN_THREADS), win_bytes, stream, G);
    if (ev_mid) SGS_HIP(ctx, hipEventRecord(ev_mid, stream));
    // level 2: super-tile queues -> tile queues (count, scan of the tile counters + render order, emit)
    const unsigned exp_grid = (unsigned)std::min<int64_t>(std::max(64, ctx->exp_grid / nf), (int64_t)ns + (P.n + SGS_SEG - 1) / SGS_SEG);
    if (bin) hipLaunchKernelGGL((sgs::k_expand<false>), dim3(std::max(1u, exp_grid), F), dim3(SGS_EXP_THREADS), 0, stream, G);
    // one workgroup per SGS_SCAN_THREADS tiles of the band (16 at 1080p, 64 at 3840x2160), independent of each other
    const unsigned scan_groups = std::max(1u, ((unsigned)((row_end - row_begin) * gx) + SGS_SCAN_THREADS - 1) / SGS_SCAN_THREADS);
    hipLaunchKernelGGL(sgs::k_tile_scan, dim3(scan_groups, F), dim3(SGS_SCAN_THREADS), 0, stream, G);
    if (bin) hipLaunchKernelGGL((sgs::k_expand<true>), dim3(std::max(1u, exp_grid), F), dim3(SGS_EXP_THREADS), 0, stream, G);
    return SGS_OK;
}
// the final transmittance of stopped pixels (one more add per pixel and splat) only where something reads it
bool need_tf_of(const sgs_config& cfg, const float* out_aux) { return out_aux || cfg.bg[0] != 0.f || cfg.bg[1] != 0.f || cfg.bg[2] != 0.f; }
// S5 + S6: one workgroup per tile of the band
void launch_composite(const FrameGroup& G, int nf, hipStream_t stream, bool aux, bool count_df, bool need_tf) {
    const FrameParams& P = G.s[0].P;
    const unsigned F = (unsigned)nf, ntiles = (unsigned)((P.row_end - P.row_begin) * P.gx);
    if (ntiles == 0) return;
    const unsigned grid = ((ntiles + 7u) / 8u) * 8u;
    // (D_f is counted only on request: the per-pixel bookkeeping and the end-of-tile reduction cost ~4 % of a sweep)
    if (aux) {
        if (count_df) hipLaunchKernelGGL((sgs::k_tile_render<true, true, true>), dim3(grid, F), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_tile_render<true, false, true>), dim3(grid, F), dim3(256), 0, stream, G);
    } else if (need_tf) {
        if (count_df) hipLaunchKernelGGL((sgs::k_tile_render<false, true, true>), dim3(grid, F), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_tile_render<false, false, true>), dim3(grid, F), dim3(256), 0, stream, G);
    } else {
        if (count_df) hipLaunchKernelGGL((sgs::k_tile_render<false, true, false>), dim3(grid, F), dim3(256), 0, stream, G);
        else hipLaunchKernelGGL((sgs::k_tile_render<false, false, false>), dim3(grid, F), dim3(256), 0, stream, G);
    }
}

// How a group of frames is issued: which stream its launches go to, and who does the runtime calls around them.
//                   stream                       forked from the caller's by   status slots cleared / copied back by   `done` recorded
//   caller          the caller's                 -                             enqueue_group                            -
//   lane            lane `lane0`'s own           enqueue_group                 enqueue_group                            by enqueue_group, on the lane's stream
//   batch_lanes     lane `stream_lane`'s own     the batch, once per chunk     the batch, once per chunk                - (the batch waits for the streams)
//   batch_caller    the caller's                 -                             the batch, once per chunk                -
// On the caller's stream (caller, batch_caller) the group first waits for the `done` of every lane it uses that is still busy with a
// pipelined frame.  caller: ordinary frames; lane: SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED single frames; batch_lanes: sgs_render_batch*;
// batch_caller: sgs_render_batch* under the SGS_FLAG_FULL_SORT test hook.  (The per-frame runtime calls around the launches were ~40 us,
// as long as a light band of tile rows takes on the GPU: hence once per chunk in a batch.)
enum class Issue { caller, lane, batch_lanes, batch_caller };

// A GROUP of nf <= SGS_MAX_GROUP frames of one scene — same resolution, same band, one camera each — issued as ONE set of launches
// (blockIdx.y = frame; sgs_common.h FrameGroup).  Frame f uses the intermediates of lane lane0 + f and status slot slot0 + f, and
// writes outs[f].  nf = 1 and lane0 = 0 for Issue::caller, nf = 1 for Issue::lane; timed and out_aux are single-frame facilities.
struct Group {
    const sgs_scene* scene; const sgs_camera* cams; int nf; const sgs_config* cfg; Band band;
    float* const* outs; float* out_aux;
    int slot0, lane0;
    int stream_lane;                         // Issue::batch_lanes: the lane whose stream the group runs on
    hipStream_t caller_stream;
    bool timed;
    Issue mode;
};

// The FrameGroup of g: the lanes' intermediates are grown here if need be.
int build_group(sgs_ctx* ctx, FrameGroup& G, const Group& g) {
    int rc;
    const sgs_scene* scene = g.scene;
    const int cp = SGS_TILE >> g.band.z;          // (the frames of a group share a resolution, a configuration and the fine-tile shift)
    const int gx = (g.cams->width + cp - 1) / cp, gy = (g.cams->height + cp - 1) / cp;
    memset(&G, 0, sizeof G);
    G.geom = scene->geom.p; G.shq = scene->shq.p; G.cbound = scene->cbound.p; G.inv = scene->inv.p; G.row_acc = ctx->row_acc.p;
    for (int f = 0; f < g.nf; ++f) {
        Lane& A = ctx->lanes[g.lane0 + f];
        if ((rc = ensure_splats(ctx, A, scene->n)) != SGS_OK) return rc;
        if ((rc = ensure_tiles(ctx, A, gx * gy)) != SGS_OK) return rc;
        if ((rc = ensure_records(ctx, A)) != SGS_OK) return rc;
        FrameSlot& S = G.s[f];
        fill_params(S.P, ctx, A, scene, &g.cams[f], *g.cfg, g.band);
        if ((S.P.flags & SGS_FLAG_FULL_SORT) && (rc = ensure_sorted_out(ctx, A)) != SGS_OK) return rc;
        S.splats = A.splats.p; S.vismask = A.vismask.p; S.bigmask = A.bigmask.p; S.big_list = A.big_list.p; S.binrec = A.binrec.p;
        S.live_list = A.live_list.p;
        S.tile_count = A.tile_count.p; S.tile_offset = A.tile_offset.p; S.tile_order = A.tile_order.p;
        S.blk_list = A.blk_list.p; S.blk_len = A.blk_len.p;
        S.stile_count = A.stile_count.p; S.stile_offset = A.stile_offset.p; S.jobs = A.jobs.p; S.job_base = A.job_base.p;
        S.rec = A.rec.p; S.alt = A.alt.p; S.part = A.part.p; S.sorted_out = A.sorted_out.p;
        S.tile_prof = A.tile_prof.p; S.bin_prof = A.bin_prof.p;
        S.out_rgb = g.outs[f]; S.out_aux = g.out_aux; S.st = ctx->ring.d_status.p + g.slot0 + f;
    }
    return SGS_OK;
}

// Enqueue the group g (Issue says on which stream and with which calls around the launches).  `first` = the record of its frame 0; frame
// f's differs by slot + f and lane + f alone.
int enqueue_group(sgs_ctx* ctx, const Group& g, FrameRec& first) {
    int rc;
    const bool own_stream = g.mode == Issue::lane || g.mode == Issue::batch_lanes;
    const bool in_batch = g.mode == Issue::batch_lanes || g.mode == Issue::batch_caller;
    const int nf = g.nf;
    // The stream: a pipelined frame's own lane's; a batch's groups rotate over the streams of lanes 0 .. group_lanes-1 — the
    // SAME streams single pipelined frames use.  (r03y: the groups used to run on the streams of lanes 0 and 4; a process that
    // had issued one batch and then pipelined single frames owned four lane streams + the caller's, the runtime maps streams onto
    // four hardware queues, two lanes shared one and the sweep was 11 % slower — 4180 vs 3750 frames/s — for the rest of the process.)
    Lane& L = ctx->lanes[g.mode == Issue::batch_lanes ? g.stream_lane : g.lane0];
    hipStream_t stream = g.caller_stream;
    if (own_stream) {
        if ((rc = ensure_lane_stream(ctx, L)) != SGS_OK) return rc;
        stream = L.stream.s;
    }
    FrameGroup G;
    if ((rc = build_group(ctx, G, g)) != SGS_OK) return rc;
    const FrameParams& P = G.s[0].P;
    if (g.mode == Issue::lane) {
        // start after whatever the caller already put on its stream (scene upload, consumers of the output buffer)
        SGS_HIP(ctx, hipEventRecord(L.fork.e, g.caller_stream));
        SGS_HIP(ctx, hipStreamWaitEvent(L.stream.s, L.fork.e, 0));
    } else if (!own_stream) {
        for (int f = 0; f < nf; ++f)               // these lanes' buffers may still be in use by a pipelined frame
            if (ctx->lanes[g.lane0 + f].busy) SGS_HIP(ctx, hipStreamWaitEvent(g.caller_stream, ctx->lanes[g.lane0 + f].done.e, 0));
    }
    StatusRing& R = ctx->ring;
    FrameStatus* st = R.d_status.p + g.slot0;
    if (!in_batch) SGS_HIP(ctx, hipMemsetAsync(st, 0, sizeof(FrameStatus) * (size_t)nf, stream));
    const bool timed = g.timed;
    const sgs::Event* ev = nullptr;
    if (timed) {
        if ((rc = ensure_timing_events(ctx)) != SGS_OK) return rc;
        ev = R.events(g.slot0);
    }
    for (int f = 0; f < nf; ++f) R.timed[g.slot0 + f] = timed && f == 0;
    if (timed) SGS_HIP(ctx, hipEventRecord(ev[0].e, stream));

    launch_project(ctx, G, nf, stream);
    if (timed) SGS_HIP(ctx, hipEventRecord(ev[1].e, stream));
    launch_binning(ctx, G, nf, stream, timed ? ev[2].e : nullptr);
    if (timed) SGS_HIP(ctx, hipEventRecord(ev[3].e, stream));
    launch_composite(G, nf, stream, g.out_aux != nullptr, (g.cfg->flags & SGS_FLAG_STATS) != 0, need_tf_of(*g.cfg, g.out_aux));
    if (timed) SGS_HIP(ctx, hipEventRecord(ev[4].e, stream));
    SGS_HIP(ctx, hipGetLastError());
    if (!in_batch) {
        SGS_HIP(ctx, hipMemcpyAsync(R.h_status.p + g.slot0, st, sizeof(FrameStatus) * (size_t)nf, hipMemcpyDeviceToHost, stream));
        if (g.mode == Issue::lane) {
            SGS_HIP(ctx, hipEventRecord(L.done.e, L.stream.s));
            L.busy = true;
        }
    }

    first = FrameRec();
    first.slot = g.slot0; first.lane = g.lane0; first.stream = g.caller_stream; first.timed = timed;
    first.scene = g.scene; first.n = g.scene->n; first.sh_rows = g.scene->sh_rows;
    first.pixels = g.band.pixel_rows * g.cams->width;
    first.T = P.gx * P.gy; first.t_lo = P.row_begin * P.gx; first.t_hi = P.row_end * P.gx; first.tiles = first.t_hi - first.t_lo;
    return SGS_OK;
}

// The record capacity an overflowed frame is known to need: its D when level 2 of the binning counted it, and twice its D_s (the
// super-tile queues take half the capacity) — an overflow at level 1 leaves d_total at 0.
int64_t records_needed(const FrameStatus& s) { return std::max<int64_t>((int64_t)s.d_total, 2 * (int64_t)s.ds_total); }

// Fill `stats` from the (already synchronised) status of the frame r.
void collect(const StatusRing& R, const FrameRec& r, sgs_stats* stats) {
    if (!stats) return;
    const FrameStatus& s = R.h_status.p[r.slot];
    const int64_t n = r.n, pixels = r.pixels;
    const int sh_rows = r.sh_rows;
    memset(stats, 0, sizeof *stats);
    stats->n_gaussians = n;
    stats->n_visible = s.n_visible;
    stats->d_total = s.d_total;
    stats->d_fetched = (int64_t)s.d_fetched;
    stats->n_pixels = pixels;
    stats->n_tiles = r.tiles;
    stats->max_tile_len = (int32_t)s.max_tile_len;
    stats->n_spill_tiles = (int32_t)s.class_count[3];
    stats->n_deep_windows = (int64_t)s.n_deep;
    stats->retries = r.retries;
    // Algorithmic bytes per stage — DESIGN.md §4 (what the stage must move, not what it happens to).
    const int64_t nv = s.n_visible, D = s.d_total, Df = (int64_t)s.d_fetched;
    stats->bytes[SGS_STAGE_PREPROCESS] = 16 * n + (32 + 16 * (int64_t)sh_rows + 64 + 16) * nv;   // rows read; splat + binning record written
    // two-level binning (D_s = records in the super-tile queues): level 1 reads every visible splat's 16-B binning record in
    // both of its passes and writes D_s of them; level 2 reads those in both of its passes and writes the D 8-B tile records
    const int64_t Ds = s.ds_total;
    stats->d_super = Ds;
    stats->bytes[SGS_STAGE_COUNT] = 2 * 16 * nv + 16 * Ds;
    stats->bytes[SGS_STAGE_EMIT] = 2 * 16 * Ds + 8 * D + 8 * ((int64_t)r.T + 1);
    stats->bytes[SGS_STAGE_RENDER] = 8 * D + 36 * Df + 12 * pixels;               // every record seen once, D_f splats blended
    if (r.timed && R.ev) {
        const sgs::Event* ev = R.events(r.slot);
        for (int i = 0; i < SGS_NUM_STAGES; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i].e, ev[i + 1].e) == hipSuccess) stats->ms[i] = ms;
        }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[0].e, ev[SGS_NUM_STAGES].e) == hipSuccess) stats->ms_total = ms;
    }
}

}  // namespace

extern "C" {

int sgs_version(void) { return SGS_VERSION; }

void sgs_struct_sizes(int32_t* camera_bytes, int32_t* config_bytes, int32_t* stats_bytes) {
    if (camera_bytes) *camera_bytes = (int32_t)sizeof(sgs_camera);
    if (config_bytes) *config_bytes = (int32_t)sizeof(sgs_config);
    if (stats_bytes) *stats_bytes = (int32_t)sizeof(sgs_stats);
}

void sgs_config_default(sgs_config* cfg) {
    if (!cfg) return;
    cfg->near_z = 0.2f; cfg->far_z = 1.0e30f; cfg->dilation = 0.3f; cfg->clamp = 1.3f;
    cfg->alpha_min = 1.0f / 255.0f; cfg->alpha_max = 0.99f; cfg->t_min = 1.0e-4f;
    cfg->bg[0] = cfg->bg[1] = cfg->bg[2] = 0.f;
    cfg->sh_degree = -1; cfg->flags = 0;
    cfg->tile_row_stride = 1; cfg->tile_row_phase = 0;
}

const char* sgs_last_error(const sgs_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sgs_create(int device_id, int backend, sgs_ctx** out) {
    if (!out) { g_create_error = "sgs_create: out is NULL"; return SGS_ERR_INVALID; }
    *out = nullptr;
    if (backend != SGS_BACKEND_HIP) {
        g_create_error = "sgs_create: only SGS_BACKEND_HIP exists; the CPU restatement lives in oracle/ (tests only)";
        return SGS_ERR_BACKEND;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = std::string("sgs_create: no HIP device (") + hipGetErrorString(e) + ")";
        return SGS_ERR_HIP;
    }
    if (device_id < 0 || device_id >= count) { g_create_error = "sgs_create: device_id out of range"; return SGS_ERR_INVALID; }
    sgs_ctx* ctx = new (std::nothrow) sgs_ctx;
    if (!ctx) { g_create_error = "sgs_create: out of host memory"; return SGS_ERR_OOM; }
    ctx->device = device_id;
    auto fail = [&](const char* what, hipError_t err) {
        g_create_error = std::string("sgs_create: ") + what + ": " + hipGetErrorString(err);
        sgs_destroy(ctx);
        return SGS_ERR_HIP;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = ctx->ring.d_status.grow(kStatusRing)) != hipSuccess) return fail("the status ring", e);
    if ((e = ctx->ring.h_status.grow(kStatusRing)) != hipSuccess) return fail("the pinned status ring", e);
    if ((e = ctx->row_acc.grow(SGS_MAX_ROWS)) != hipSuccess) return fail("the row counters", e);
    if ((e = hipMemset(ctx->row_acc.p, 0, sizeof(unsigned long long) * SGS_MAX_ROWS)) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return fail("hipStreamSynchronize", e);
    // (nothing is read from the environment: sgs_set_tuning is the library's whole tuning surface)
    *out = ctx;
    return SGS_OK;
}

int sgs_destroy(sgs_ctx* ctx) {
    if (!ctx) return SGS_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
    return SGS_OK;
}

void sgs_tuning_default(sgs_tuning* out) {
    if (!out) return;
    out->lanes = 3; out->group = 8; out->group_lanes = 2; out->morton = 1; out->record_capacity = 16ll << 20;
    out->fine_tile_pixels = 640 * 480; out->fine_tile_growth = 2.2;
}

int sgs_get_tuning(const sgs_ctx* ctx, sgs_tuning* out) {
    if (!ctx || !out) return SGS_ERR_INVALID;
    out->lanes = ctx->n_lanes; out->group = ctx->group; out->group_lanes = ctx->group_lanes; out->morton = ctx->morton ? 1 : 0;
    out->record_capacity = ctx->rec_cap_wanted; out->fine_tile_pixels = ctx->fine_tile_pixels; out->fine_tile_growth = ctx->fine_tile_growth;
    return SGS_OK;
}

int sgs_set_tuning(sgs_ctx* ctx, const sgs_tuning* t) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!t) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_set_tuning: tuning is NULL");
    if (t->lanes < 1 || t->lanes > kMaxLanes) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.lanes %d outside [1, %d]", t->lanes, kMaxLanes);
    if (t->group < 1 || t->group > std::min(kMaxLanes, SGS_MAX_GROUP)) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.group %d outside [1, %d]", t->group, std::min(kMaxLanes, SGS_MAX_GROUP));
    if (t->group_lanes < 1 || t->group * t->group_lanes > kMaxLanes)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.group x group_lanes = %d x %d exceeds the %d lanes of a context", t->group, t->group_lanes, kMaxLanes);
    if (t->record_capacity <= 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.record_capacity must be positive");
    if (t->fine_tile_pixels < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.fine_tile_pixels must not be negative (0 = never)");
    if (!(t->fine_tile_growth >= 1.0)) SGS_FAIL(ctx, SGS_ERR_INVALID, "sgs_tuning.fine_tile_growth must be at least 1 (>= 16: whenever the pixel rule allows)");
    // the capacity first: it is the one field that can still be refused (its own limit, an allocation); a refused tuning changes nothing
    if (t->record_capacity != ctx->rec_cap_wanted) {
        const int rc = sgs_set_record_capacity(ctx, t->record_capacity);
        if (rc != SGS_OK) return rc;
    } else {
        SGS_HIP(ctx, hipSetDevice(ctx->device));
        SGS_HIP(ctx, hipDeviceSynchronize());              // frames in flight were issued under the old values (their verdicts stay for sgs_frame_sync)
    }
    ctx->n_lanes = t->lanes; ctx->next_lane = 0; ctx->group = t->group; ctx->group_lanes = t->group_lanes; ctx->morton = t->morton != 0;
    ctx->fine_tile_pixels = t->fine_tile_pixels; ctx->fine_tile_growth = t->fine_tile_growth;
    return SGS_OK;
}

int sgs_set_record_capacity(sgs_ctx* ctx, int64_t max_records) {
    if (!ctx) return SGS_ERR_INVALID;
    if (max_records <= 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "max_records must be positive");
    if (max_records > kMaxRecords) SGS_FAIL(ctx, SGS_ERR_INVALID, "record capacity %lld exceeds 2^32", (long long)max_records);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    SGS_HIP(ctx, hipDeviceSynchronize());
    const int64_t prev = ctx->rec_cap_wanted;
    ctx->rec_cap_wanted = max_records;
    for (Lane& L : ctx->lanes) release_records(L);      // reallocated at the requested size (lanes other than 0: on next use)
    // the new capacity holds only once lane 0's buffers exist; a failed allocation leaves the previous one wanted (every lane
    // reallocates at it on its next frame)
    const int rc = ensure_records(ctx, ctx->lanes[0]);
    if (rc != SGS_OK) ctx->rec_cap_wanted = prev;
    return rc;
}

namespace {

// The device side of a scene load (sgs_kernels.h "Upload"): Z-order permutation of the means by a radix sort on the device, layout
// (dequantising when the source is the compressed payload), per-chunk bounds.  src = the five fp32 arrays on the device, or Z.
int layout_scene(sgs_ctx* ctx, sgs_scene* sc, const float* const* src, const sgs::PackedScene& Z, bool packed) {
    const int64_t n = sc->n;
    const int nf = 3 * (sc->sh_degree + 1) * (sc->sh_degree + 1);
    const size_t npad = (size_t)std::max<int64_t>(sc->n_chunks, 1) * 64;
    DevBuf<unsigned long long> own_keys[2];       // the sort's buffers: released when this returns, however it returns
    DevBuf<unsigned> own_idx[2], own_hist, own_bounds;
    unsigned long long* keys[2] = {nullptr, nullptr};
    unsigned* idx[2] = {nullptr, nullptr};
    const unsigned* d_perm = nullptr;
    const float* means = packed ? nullptr : src[0];
    if (ctx->morton && n > SGS_WAVE) {
        // Z-order (Morton) permutation of the means, once per scene: 64 consecutive Gaussians then occupy a compact cell, so a chunk is
        // visible or culled as a whole (no half-used SH cache lines in k_preprocess) and its splats overlap on screen (binning)
        const unsigned nblocks = (unsigned)((n + SGS_RSORT_TILE - 1) / SGS_RSORT_TILE);
        for (int k = 0; k < 2; ++k) {
            SGS_HIP(ctx, own_keys[k].grow(n));
            SGS_HIP(ctx, own_idx[k].grow(n));
            keys[k] = own_keys[k].p; idx[k] = own_idx[k].p;
        }
        const unsigned nscan = (256u * nblocks + SGS_RSCAN_SPAN - 1) / SGS_RSCAN_SPAN;          // (hist, then k_radix_scan's span sums)
        SGS_HIP(ctx, own_hist.grow((int64_t)256 * nblocks + nscan));
        SGS_HIP(ctx, own_bounds.grow(6));
        unsigned* const hist = own_hist.p;
        unsigned* const bounds = own_bounds.p;
        const unsigned init[6] = {~0u, ~0u, ~0u, 0u, 0u, 0u};
        SGS_HIP(ctx, hipMemcpy(bounds, init, sizeof init, hipMemcpyHostToDevice));
        const unsigned g1 = (unsigned)std::min<int64_t>(512, (n + 255) / 256), gn = (unsigned)((n + 255) / 256);
        if (packed) {
            hipLaunchKernelGGL((sgs::k_mean_bounds<true>), dim3(g1), dim3(256), 0, 0, (long long)n, means, Z, bounds);
            hipLaunchKernelGGL((sgs::k_morton_keys<true>), dim3(gn), dim3(256), 0, 0, (long long)n, means, Z, bounds, keys[0], idx[0]);
        } else {
            hipLaunchKernelGGL((sgs::k_mean_bounds<false>), dim3(g1), dim3(256), 0, 0, (long long)n, means, Z, bounds);
            hipLaunchKernelGGL((sgs::k_morton_keys<false>), dim3(gn), dim3(256), 0, 0, (long long)n, means, Z, bounds, keys[0], idx[0]);
        }
        int cur = 0;
        for (int shift = 0; shift < 64; shift += 8, cur ^= 1) {      // 63 key bits: eight stable passes
            hipLaunchKernelGGL(sgs::k_radix_count, dim3(nblocks), dim3(256), 0, 0, (long long)n, keys[cur], shift, nblocks, hist);
            hipLaunchKernelGGL(sgs::k_radix_scan, dim3(nscan), dim3(1024), 0, 0, 256u * nblocks, hist, hist + (size_t)256 * nblocks);
            hipLaunchKernelGGL(sgs::k_radix_scatter, dim3(nblocks), dim3(256), 0, 0, (long long)n, keys[cur], idx[cur], keys[cur ^ 1], idx[cur ^ 1],
                               shift, nblocks, hist, hist + (size_t)256 * nblocks);
        }
        d_perm = idx[cur];                 // (an even number of passes: back in buffer 0)
        sc->perm_host.resize((size_t)n);
        SGS_HIP(ctx, hipMemcpy(sc->perm_host.data(), d_perm, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    {
        const unsigned grid = (unsigned)((npad + 255) / 256);
        if (packed)
            hipLaunchKernelGGL((sgs::k_scene_layout<true>), dim3(grid), dim3(256), 0, 0, (long long)n, nf, sc->sh_rows, d_perm,
                               nullptr, nullptr, nullptr, nullptr, nullptr, Z, sc->geom.p, sc->shq.p);
        else
            hipLaunchKernelGGL((sgs::k_scene_layout<false>), dim3(grid), dim3(256), 0, 0, (long long)n, nf, sc->sh_rows, d_perm,
                               src[0], src[1], src[2], src[3], src[4], Z, sc->geom.p, sc->shq.p);
        hipLaunchKernelGGL(sgs::k_chunk_bounds, dim3((unsigned)((sc->n_chunks + 3) / 4)), dim3(256), 0, 0, (long long)n,
                           (long long)sc->n_chunks, sc->geom.p, sc->cbound.p);
        SGS_HIP(ctx, hipDeviceSynchronize());
    }
    if (n > 0) {
        // the probe (fine_shift_of): a pre-sample of up to 64 Ki Gaussians at even strides through the caller's order comes to the host (through
        // the inverse of the Z-order permutation, made in the sort's spare index buffer, which the scene then keeps: the composite finds a
        // splat's record through it); 512 of them are drawn from it — systematically, with
        // probability 1/2 (1 / M0 + trace_i / sum of traces) each — and their covariances formed once
        const int M0 = (int)std::min<int64_t>(n, 65536), M = std::min(M0, 512);
        DevBuf<float4> own_probe;
        unsigned* d_inv = nullptr;
        if (d_perm) {
            d_inv = idx[d_perm == idx[0] ? 1 : 0];
            hipLaunchKernelGGL(sgs::k_invert_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, d_perm, d_inv);
        }
        std::vector<float4> rows((size_t)M0 * SGS_GEOM_ROWS);
        SGS_HIP(ctx, own_probe.grow((int64_t)rows.size()));
        float4* const d_probe = own_probe.p;
        hipLaunchKernelGGL(sgs::k_probe_gather, dim3((unsigned)((M0 + 255) / 256)), dim3(256), 0, 0, (long long)n, M0, d_inv, sc->geom.p, d_probe);
        SGS_HIP(ctx, hipMemcpy(rows.data(), d_probe, rows.size() * sizeof(float4), hipMemcpyDeviceToHost));
        own_probe.reset();
        if (d_inv) sc->inv = std::move(own_idx[d_inv == idx[0] ? 0 : 1]);      // (the copy above has waited for k_invert_perm; one owner: the scene)
        {
            std::vector<double> tr((size_t)M0);
            double T = 0.0;
            for (int i = 0; i < M0; ++i) {
                const float4 g1 = rows[(size_t)3 * i + 1];
                const double t = (double)g1.x * g1.x + (double)g1.y * g1.y + (double)g1.z * g1.z;       // trace(R S S^T R^T) = |s|^2
                tr[(size_t)i] = t < 1.0e30 ? t : 0.0;                                                 // (NaN / inf scales: never drawn by size)
                T += tr[(size_t)i];
            }
            sc->probe.clear(); sc->probe.reserve((size_t)M);
            double cum = 0.0; int i = 0;
            for (int k = 0; k < M; ++k) {
                double pi_i = 1.0 / M0;
                if (M0 > M) {              // (a scene smaller than a probe: every Gaussian once, weight 1)
                    const double target = ((double)k + 0.5) / M;
                    for (;;) {
                        pi_i = 0.5 * (1.0 / M0 + (T > 0.0 ? tr[(size_t)i] / T : 1.0 / M0));
                        if (cum + pi_i >= target || i == M0 - 1) break;
                        cum += pi_i; ++i;
                    }
                } else i = k;
                const float4 g0 = rows[(size_t)3 * i], g1 = rows[(size_t)3 * i + 1], g2 = rows[(size_t)3 * i + 2];
                ProbeSample q;
                q.m[0] = g0.x; q.m[1] = g0.y; q.m[2] = g0.z; q.ln_o = std::log(g0.w);
                q.wgt = (float)(1.0 / (pi_i * M0));                       // (relative to a uniform draw)
                const double qn = std::sqrt((double)g1.w * g1.w + (double)g2.x * g2.x + (double)g2.y * g2.y + (double)g2.z * g2.z);
                const double w = g1.w / qn, x = g2.x / qn, y = g2.y / qn, z = g2.z / qn;
                const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)},
                                        {2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)},
                                        {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)}};
                const double s2[3] = {(double)g1.x * g1.x, (double)g1.y * g1.y, (double)g1.z * g1.z};
                int t = 0;
                for (int a_ = 0; a_ < 3; ++a_)
                    for (int b_ = a_; b_ < 3; ++b_)
                        q.S[t++] = (float)(R[a_][0] * R[b_][0] * s2[0] + R[a_][1] * R[b_][1] * s2[1] + R[a_][2] * R[b_][2] * s2[2]);     // (00, 01, 02, 11, 12, 22)
                q.trace = q.S[0] + q.S[3] + q.S[5];
                sc->probe.push_back(q);
            }
        }
    }
    return SGS_OK;
}

// a new scene object with its device buffers
int new_scene(sgs_ctx* ctx, int64_t n, int sh_degree, bool sh_packed, std::unique_ptr<sgs_scene>& out) {
    std::unique_ptr<sgs_scene> sc(new (std::nothrow) sgs_scene);
    if (!sc) SGS_FAIL(ctx, SGS_ERR_OOM, "out of host memory");
    const int nf = 3 * (sh_degree + 1) * (sh_degree + 1);
    sc->n = n; sc->n_chunks = (n + 63) / 64; sc->sh_degree = sh_degree; sc->sh_packed = sh_packed;
    sc->sh_rows = sh_packed ? (12 + (nf - 3) + 15) / 16 : (nf + 3) / 4;      // packed: 12 B of fp32 DC + one byte per higher coefficient
    const size_t npad = (size_t)std::max<int64_t>(sc->n_chunks, 1) * 64;
    SGS_HIP(ctx, sc->geom.grow((int64_t)(npad * SGS_GEOM_ROWS)));
    SGS_HIP(ctx, sc->shq.grow((int64_t)(npad * sc->sh_rows)));
    SGS_HIP(ctx, sc->cbound.grow((int64_t)(npad / 64) * 2));
    out = std::move(sc);
    return SGS_OK;
}

// host arrays -> device copies (on_device: the caller's pointers as they are).  staged[] owns the copies.
int stage(sgs_ctx* ctx, int on_device, const void* const* src, const size_t* bytes, int count, const void** dev, DevBuf<unsigned char>* staged) {
    for (int i = 0; i < count; ++i) {
        if (on_device || !src[i] || bytes[i] == 0) { dev[i] = src[i]; continue; }
        SGS_HIP(ctx, staged[i].grow((int64_t)bytes[i]));
        SGS_HIP(ctx, hipMemcpy(staged[i].p, src[i], bytes[i], hipMemcpyHostToDevice));
        dev[i] = staged[i].p;
    }
    return SGS_OK;
}

}  // namespace

int sgs_scene_upload(sgs_ctx* ctx, int64_t n, int sh_degree, const float* means, const float* scales,
                     const float* quats, const float* opacities, const float* sh, int on_device,
                     sgs_scene** out) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!out) SGS_FAIL(ctx, SGS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n < 0 || n > 0x7fffffffll) SGS_FAIL(ctx, SGS_ERR_INVALID, "n = %lld out of range", (long long)n);
    if (sh_degree < 0 || sh_degree > 3) SGS_FAIL(ctx, SGS_ERR_INVALID, "sh_degree %d not in 0..3", sh_degree);
    if (n > 0 && (!means || !scales || !quats || !opacities || !sh)) SGS_FAIL(ctx, SGS_ERR_INVALID, "null input array");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sgs_scene> sc;            // (released with its buffers by any return before *out)
    int rc;
    if ((rc = new_scene(ctx, n, sh_degree, false, sc)) != SGS_OK) return rc;
    if (n > 0) {
        const int nf = 3 * (sh_degree + 1) * (sh_degree + 1);
        const void* src[5] = {means, scales, quats, opacities, sh};
        const size_t bytes[5] = {(size_t)n * 12, (size_t)n * 12, (size_t)n * 16, (size_t)n * 4, (size_t)n * nf * 4};
        const void* dev[5]; DevBuf<unsigned char> staged[5];
        if ((rc = stage(ctx, on_device, src, bytes, 5, dev, staged)) != SGS_OK) return rc;
        const float* f[5] = {(const float*)dev[0], (const float*)dev[1], (const float*)dev[2], (const float*)dev[3], (const float*)dev[4]};
        sgs::PackedScene Z = {nullptr, nullptr, nullptr, 0};
        if ((rc = layout_scene(ctx, sc.get(), f, Z, false)) != SGS_OK) return rc;
    }
    *out = sc.release();
    return SGS_OK;
}

int sgs_scene_upload_compressed(sgs_ctx* ctx, const sgs_compressed_scene* z, int on_device, sgs_scene** out) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!out || !z) SGS_FAIL(ctx, SGS_ERR_INVALID, "null argument");
    *out = nullptr;
    const int64_t n = z->n;
    if (n < 0 || n > 0x7fffffffll) SGS_FAIL(ctx, SGS_ERR_INVALID, "n = %lld out of range", (long long)n);
    if (z->sh_degree < 0 || z->sh_degree > 3) SGS_FAIL(ctx, SGS_ERR_INVALID, "sh_degree %d not in 0..3", z->sh_degree);
    const int k_rest = (z->sh_degree + 1) * (z->sh_degree + 1) - 1;
    if (z->sh_decode < SGS_SH_DECODE_UNSPECIFIED || z->sh_decode > SGS_SH_DECODE_BIN_CENTRE) SGS_FAIL(ctx, SGS_ERR_INVALID, "sh_decode %d is not one of SGS_SH_DECODE_*", z->sh_decode);
    if (k_rest > 0 && z->sh_decode == SGS_SH_DECODE_UNSPECIFIED)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "sh_decode is required for a scene with 8-bit SH coefficients (sh_degree %d): SGS_SH_DECODE_BIN_CENTRE, _LINEAR255 or "
                                       "_BIN_CENTRE_ENDS — there is no default, include/sage_gs.h says why", z->sh_degree);
    if (n > 0 && (!z->chunks || !z->packed || (k_rest > 0 && !z->sh))) SGS_FAIL(ctx, SGS_ERR_INVALID, "null input array");
    if (z->n_chunks != (n + 255) / 256) SGS_FAIL(ctx, SGS_ERR_INVALID, "n_chunks %lld is not ceil(n / 256)", (long long)z->n_chunks);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sgs_scene> sc;
    int rc;
    if ((rc = new_scene(ctx, n, z->sh_degree, true, sc)) != SGS_OK) return rc;
    // (the kernels' mode: 0 = bin centre — one exact fma —, 1 = linear255, 2 = bin centre with exact ends)
    sc->sh_decode = (z->sh_decode == SGS_SH_DECODE_BIN_CENTRE || z->sh_decode == SGS_SH_DECODE_UNSPECIFIED) ? 0 : z->sh_decode;
    if (n > 0) {
        const void* src[3] = {z->chunks, z->packed, z->sh};
        const size_t bytes[3] = {(size_t)z->n_chunks * 18 * 4, (size_t)n * 16, (size_t)n * 3 * k_rest};
        const void* dev[3]; DevBuf<unsigned char> staged[3];
        if ((rc = stage(ctx, on_device, src, bytes, 3, dev, staged)) != SGS_OK) return rc;
        sgs::PackedScene Z = {(const float*)dev[0], (const uint4*)dev[1], (const unsigned char*)dev[2], k_rest};
        if ((rc = layout_scene(ctx, sc.get(), nullptr, Z, true)) != SGS_OK) return rc;
    }
    *out = sc.release();
    return SGS_OK;
}

int sgs_scene_free(sgs_ctx* ctx, sgs_scene* scene) {
    if (!scene) return SGS_OK;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipDeviceSynchronize(); }
    if (ctx && ctx->last.scene == scene) ctx->last.scene = nullptr;
    delete scene;
    return SGS_OK;
}

int sgs_frame_sync(sgs_ctx* ctx, sgs_stats* stats) {
    if (!ctx) return SGS_ERR_INVALID;
    if (ctx->last.slot < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "no frame has been issued");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    SGS_HIP(ctx, hipStreamSynchronize(ctx->last.stream));
    { int rc_ = drain_lanes(ctx); if (rc_ != SGS_OK) return rc_; }
    StatusRing& R = ctx->ring;
    collect(R, ctx->last, stats);
    // every frame issued since the previous synchronisation is checked, not just the last one
    int bad = -1, n_bad = 0;
    double ms_sum[SGS_NUM_STAGES + 1] = {};
    int n_timed = 0;
    R.for_pending([&](int slot) {
        if (R.h_status.p[slot].overflow) { bad = slot; ++n_bad; }
        if (R.timed[slot] && R.ev) {
            const sgs::Event* ev = R.events(slot);
            float ms = 0.f;
            for (int i = 0; i < SGS_NUM_STAGES; ++i)
                if (hipEventElapsedTime(&ms, ev[i].e, ev[i + 1].e) == hipSuccess) ms_sum[i] += ms;
            if (hipEventElapsedTime(&ms, ev[0].e, ev[SGS_NUM_STAGES].e) == hipSuccess) ms_sum[SGS_NUM_STAGES] += ms;
            ++n_timed;
        }
    });
    if (stats && n_timed > 1) {          // several pipelined frames: report the per-frame average
        for (int i = 0; i < SGS_NUM_STAGES; ++i) stats->ms[i] = (float)(ms_sum[i] / n_timed);
        stats->ms_total = (float)(ms_sum[SGS_NUM_STAGES] / n_timed);
    }
    R.seen();
    if (n_bad)
        SGS_FAIL(ctx, SGS_ERR_OVERFLOW, "%d frame(s) overflowed the record capacity %lld (one needs at least %lld records: D = %u, D_s = %u "
                 "super-tile records of which the capacity holds half as many); call sgs_set_record_capacity", n_bad,
                 (long long)ctx->lanes[0].rec.cap, (long long)records_needed(R.h_status.p[bad]), R.h_status.p[bad].d_total, R.h_status.p[bad].ds_total);
    return SGS_OK;
}

int sgs_render_rgbd(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config* cfg_in,
                    int tile_row_begin, int tile_row_end, float* out_rgb, float* out_aux, sgs_stats* stats,
                    void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    int rc;
    // out_aux is a full-frame buffer (sage_gs.h): the compact image of interleaved rows has no depth / coverage counterpart
    if (out_aux && cfg_in && cfg_in->tile_row_stride > 1)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "out_aux with interleaved tile rows (tile_row_stride %d) is not supported", cfg_in->tile_row_stride);
    sgs_config cfg;
    if (cfg_in) cfg = *cfg_in; else sgs_config_default(&cfg);
    float* outs[1] = {out_rgb};
    Group g = {scene, cam, 1, &cfg, Band(), outs, out_aux, 0, 0, 0, static_cast<hipStream_t>(hip_stream), (cfg.flags & SGS_FLAG_TIMING) != 0, Issue::caller};
    if ((rc = validate(ctx, scene, cam, cfg_in, tile_row_begin, tile_row_end, out_rgb, g.band)) != SGS_OK) return rc;
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    const bool pipelined = (cfg.flags & SGS_FLAG_PIPELINED) && (cfg.flags & SGS_FLAG_ASYNC) && ctx->n_lanes > 1 &&
                           !(cfg.flags & SGS_FLAG_FULL_SORT);
    if (pipelined) g.mode = Issue::lane;
    StatusRing& R = ctx->ring;
    for (int retries = 0;;) {
        if (R.full() && (rc = sgs_frame_sync(ctx, nullptr)) != SGS_OK) return rc;        // the status ring is full: drain it first
        g.slot0 = R.slot();
        if (pipelined) g.lane0 = ctx->next_lane;
        FrameRec rec;
        if ((rc = enqueue_group(ctx, g, rec)) != SGS_OK) return rc;          // (the slot was not taken: nothing will write its status word)
        R.issued();
        if (pipelined) ctx->next_lane = (ctx->next_lane + 1) % ctx->n_lanes;
        rec.retries = retries;
        ctx->last = rec;
        if (cfg.flags & SGS_FLAG_ASYNC) return SGS_OK;
        rc = sgs_frame_sync(ctx, stats);
        if (rc != SGS_ERR_OVERFLOW) return rc;
        // synchronous path: grow the queues to fit and render again.  A frame can overflow at level 1 of the binning (the super-tile
        // queues hold rec_cap / 2 records of 16 bytes): level 2 then never ran and d_total is 0 — what is known is D_s
        const int64_t need = records_needed(R.h_status.p[rec.slot]);
        ctx->rec_cap_wanted = std::max<int64_t>(need + need / 4, ctx->lanes[0].rec.cap * 2);
        if ((rc = ensure_records(ctx, ctx->lanes[0])) != SGS_OK) return rc;
        if (++retries > 4) SGS_FAIL(ctx, SGS_ERR_OVERFLOW, "record capacity still too small after 4 retries");
    }
}

int sgs_render(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config* cfg,
               int tile_row_begin, int tile_row_end, float* out_rgb, sgs_stats* stats, void* hip_stream) {
    return sgs_render_rgbd(ctx, scene, cam, cfg, tile_row_begin, tile_row_end, out_rgb, nullptr, stats, hip_stream);
}

namespace {

// ---- sgs_render_batch_strided, step by step ----

// Every camera (and the stride) is validated BEFORE anything is enqueued; bands[i] = frame i's band (the fine-tile shift is a function
// of its camera).
int validate_batch(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cams, int n_cams, const sgs_config& cfg, int row_begin,
                   int row_end, const float* out_rgb, int64_t frame_stride, std::vector<Band>& bands) {
    int rc;
    for (int i = 0; i < n_cams; ++i) {
        if ((rc = validate(ctx, scene, &cams[i], &cfg, row_begin, row_end, out_rgb, bands[(size_t)i])) != SGS_OK) return rc;
        if (cams[i].width != cams[0].width || cams[i].height != cams[0].height)
            SGS_FAIL(ctx, SGS_ERR_INVALID, "the cameras of a batch must share a resolution");
    }
    if (n_cams > 1) {
        const int64_t band_floats = bands[0].pixel_rows * (int64_t)cams[0].width * 3;       // what one frame of the batch writes
        if (frame_stride < band_floats)
            SGS_FAIL(ctx, SGS_ERR_INVALID, "frame_stride %lld is smaller than the band a frame writes (%lld floats)",
                     (long long)frame_stride, (long long)band_floats);
    }
    return SGS_OK;
}

// The plan of a chunk of cn frames: its groups, in issue order — a function of cn, F = sgs_tuning.group, the number GL of group streams
// and the frames' fine-tile shifts alone.
// The chunk's frames are dealt to the group streams in EQUAL shares (the stream with an extra group finished it alone, without a
// neighbour's kernels to overlap with; more than four frames are worth a second stream), each share cut into EQUAL groups of <= F:
// 20 frames on two streams are 5,5 + 5,5 under F = 8 (not 8,2 + 8,2: the frames of a group share their reads of the scene and their
// launches, a group of two shares little).
struct PlannedGroup { int first, count, stream; };
int plan_chunk(int cn, int F, int GL, const Band* bands, PlannedGroup* plan) {
    const int n_streams = std::min(GL, (cn + 3) / 4);
    int left[kMaxLanes], todo[kMaxLanes];           // frames / groups each stream still has to issue
    for (int sidx = 0; sidx < n_streams; ++sidx) {
        left[sidx] = cn / n_streams + (sidx < cn % n_streams ? 1 : 0);
        todo[sidx] = (left[sidx] + F - 1) / F;
    }
    int n_groups = 0;
    for (int i = 0, g = 0; i < cn; ++g) {
        const int sidx = g % n_streams;
        if (left[sidx] <= 0) continue;
        if (todo[sidx] <= 0) todo[sidx] = (left[sidx] + F - 1) / F;       // (a group that ended early, below, left frames behind)
        int nf = (left[sidx] + todo[sidx] - 1) / todo[sidx];
        --todo[sidx];
        // (the frames of a group share one set of launches, hence one grid of tiles: a group ends where the fine-tile shift changes)
        for (int f = 1; f < nf; ++f) if (bands[i + f].z != bands[i].z) { nf = f; break; }
        left[sidx] -= nf;
        plan[n_groups++] = {i, nf, sidx};
        i += nf;
    }
    return n_groups;
}

// From the first enqueue of a chunk on, NO way out of the batch leaves work running that nobody waits for: going out of scope armed
// (an error return) waits for the group streams and the caller's.  The success path calls wait() itself, which disarms.
struct ChunkJoin {
    sgs_ctx* ctx; hipStream_t stream; int n_lane_streams;
    bool armed;
    hipError_t wait() {          // (every stream is waited for, whatever an earlier one returned)
        armed = false;
        hipError_t e = hipSuccess;
        for (int gl = 0; gl <= n_lane_streams; ++gl) {
            const hipError_t e1 = hipStreamSynchronize(gl < n_lane_streams ? ctx->lanes[gl].stream.s : stream);
            if (e == hipSuccess) e = e1;
        }
        return e;
    }
    ~ChunkJoin() { if (armed) (void)wait(); }
};

// Once per chunk of frames, not once per frame: zero the status slots, fork the group streams from the caller's.
int begin_chunk(sgs_ctx* ctx, int cn, int GL, bool lanes, hipStream_t stream) {
    int rc;
    SGS_HIP(ctx, hipMemsetAsync(ctx->ring.d_status.p + ctx->ring.take_chunk(), 0, sizeof(FrameStatus) * (size_t)cn, stream));
    if (!lanes) return SGS_OK;
    if ((rc = ensure_lane_stream(ctx, ctx->lanes[0])) != SGS_OK) return rc;
    SGS_HIP(ctx, hipEventRecord(ctx->lanes[0].fork.e, stream));
    for (int gl = 0; gl < GL; ++gl) {
        if ((rc = ensure_lane_stream(ctx, ctx->lanes[gl])) != SGS_OK) return rc;
        SGS_HIP(ctx, hipStreamWaitEvent(ctx->lanes[gl].stream.s, ctx->lanes[0].fork.e, 0));
    }
    return SGS_OK;
}

}  // namespace

int sgs_render_batch_strided(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cams, int n_cams,
                             const sgs_config* cfg_in, int tile_row_begin, int tile_row_end, float* out_rgb,
                             int64_t frame_stride, sgs_stats* stats, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    if (n_cams < 0 || (n_cams > 0 && !cams)) SGS_FAIL(ctx, SGS_ERR_INVALID, "bad camera array");
    sgs_config cfg;
    if (cfg_in) cfg = *cfg_in; else sgs_config_default(&cfg);
    cfg.flags &= ~(uint32_t)SGS_FLAG_TIMING;       // per-stage events are a single-frame facility
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    StatusRing& R = ctx->ring;
    int rc;
    if (!R.idle() && (rc = sgs_frame_sync(ctx, nullptr)) != SGS_OK) return rc;
    const bool lanes = !(cfg.flags & SGS_FLAG_FULL_SORT);           // own streams (the FULL_SORT test hook stays on the caller's)
    const int F = ctx->group, GL = lanes ? ctx->group_lanes : 1;
    std::vector<Band> bands((size_t)std::max(n_cams, 1));
    if ((rc = validate_batch(ctx, scene, cams, n_cams, cfg, tile_row_begin, tile_row_end, out_rgb, frame_stride, bands)) != SGS_OK) return rc;
    for (int c0 = 0; c0 < n_cams; c0 += kStatusRing) {
        const int cn = std::min(kStatusRing, n_cams - c0);
        FrameRec recs[kStatusRing];
        PlannedGroup plan[kStatusRing];
        const int n_groups = plan_chunk(cn, F, GL, &bands[(size_t)c0], plan);
        if ((rc = begin_chunk(ctx, cn, GL, lanes, stream)) != SGS_OK) return rc;
        ChunkJoin join = {ctx, stream, lanes ? GL : 0, true};
        for (int k = 0; k < n_groups; ++k) {
            const PlannedGroup& pg = plan[k];
            float* outs[SGS_MAX_GROUP];
            for (int f = 0; f < pg.count; ++f) outs[f] = out_rgb + (size_t)(c0 + pg.first + f) * (size_t)frame_stride;
            const Group g = {scene, &cams[c0 + pg.first], pg.count, &cfg, bands[(size_t)(c0 + pg.first)], outs, nullptr, pg.first, pg.stream * F,
                             pg.stream, stream, false, lanes ? Issue::batch_lanes : Issue::batch_caller};
            if ((rc = enqueue_group(ctx, g, recs[pg.first])) != SGS_OK) return rc;
            for (int f = 1; f < pg.count; ++f) { recs[pg.first + f] = recs[pg.first]; recs[pg.first + f].slot += f; recs[pg.first + f].lane += f; }
        }
        ctx->last = recs[cn - 1];
        // ... wait for the lanes and fetch every frame's status in one copy
        SGS_HIP(ctx, join.wait());
        if ((rc = drain_lanes(ctx)) != SGS_OK) return rc;           // (frames issued outside this call)
        SGS_HIP(ctx, hipMemcpy(R.h_status.p, R.d_status.p, sizeof(FrameStatus) * (size_t)cn, hipMemcpyDeviceToHost));
        // the redo's own frames take ring slots again — these (a full chunk leaves no others) — so every verdict is read out first
        bool over[kStatusRing];
        for (int i = 0; i < cn; ++i) {
            over[i] = R.h_status.p[i].overflow != 0;
            if (stats) collect(R, recs[i], stats + c0 + i);
        }
        for (int i = 0; i < cn; ++i) {
            if (!over[i]) continue;
            // redo this one frame synchronously (grows the queues), then carry on
            sgs_config c1 = cfg; c1.flags &= ~(uint32_t)(SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED);
            if ((rc = sgs_render(ctx, scene, &cams[c0 + i], &c1, tile_row_begin, tile_row_end, out_rgb + (size_t)(c0 + i) * (size_t)frame_stride,
                                 stats ? stats + c0 + i : nullptr, hip_stream)) != SGS_OK)
                return rc;
        }
    }
    return SGS_OK;
}

int sgs_render_batch(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cams, int n_cams,
                     const sgs_config* cfg_in, int tile_row_begin, int tile_row_end, float* out_rgb,
                     sgs_stats* stats, void* hip_stream) {
    const int64_t stride = n_cams > 0 && cams ? (int64_t)cams[0].width * cams[0].height * 3 : 0;       // dense frames
    return sgs_render_batch_strided(ctx, scene, cams, n_cams, cfg_in, tile_row_begin, tile_row_end, out_rgb, stride, stats, hip_stream);
}

int sgs_row_records(sgs_ctx* ctx, int64_t* out, int n_rows, int reset) {
    if (!ctx) return SGS_ERR_INVALID;
    if (n_rows < 0 || n_rows > SGS_MAX_ROWS || (n_rows > 0 && !out)) SGS_FAIL(ctx, SGS_ERR_INVALID, "bad row buffer (%d rows)", n_rows);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    // (no device-wide synchronisation: a sweep's framebuffer exchange may be in flight on another stream and must not
    //  be waited for here; the frames the caller has synchronised are complete, and that is the contract)
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "row counters");
    if (n_rows > 0) SGS_HIP(ctx, hipMemcpy(out, ctx->row_acc.p, sizeof(int64_t) * (size_t)n_rows, hipMemcpyDeviceToHost));
    if (reset) {
        SGS_HIP(ctx, hipMemset(ctx->row_acc.p, 0, sizeof(unsigned long long) * SGS_MAX_ROWS));
        SGS_HIP(ctx, hipStreamSynchronize(nullptr));      // (see ensure_tiles: the clear must not race later frames)
    }
    return SGS_OK;
}

int sgs_pack_rgba8(sgs_ctx* ctx, const float* rgb, uint8_t* rgba, int width, int height, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!rgb || !rgba || width <= 0 || height <= 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "bad pack arguments");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    const long long n = (long long)width * height;
    hipLaunchKernelGGL(sgs::k_pack_rgba8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(hip_stream), rgb, reinterpret_cast<unsigned*>(rgba), n);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

namespace {

// ---- sgs_debug_read's host-side decodes: n bytes of a buffer into host_dst, each from the device arrays as the kernels keep them ----

// the tile offsets: k_tile_scan writes those of the band it rendered (and the band's end); outside it they are constant
int read_tile_offsets(sgs_ctx* ctx, const FrameRec& r, const Lane& L, void* host_dst, int64_t n) {
    const size_t cnt = (size_t)r.T + 1;
    std::vector<unsigned> tmp(cnt);
    SGS_HIP(ctx, hipMemcpy(tmp.data(), L.tile_offset.p, cnt * 4, hipMemcpyDeviceToHost));
    const unsigned total = tmp[(size_t)r.t_hi];
    for (int64_t i = 0; (i + 1) * 4 <= n; ++i)
        ((unsigned*)host_dst)[i] = i < r.t_lo ? 0u : i >= r.t_hi ? total : tmp[(size_t)i];
    return SGS_OK;
}

// the scene's geometry rows, back in the caller's order: [N, 11]
int read_scene_geom(sgs_ctx* ctx, const sgs_scene* sc, int64_t n_slots, void* host_dst, int64_t n) {
    std::vector<float4> rows((size_t)n_slots * SGS_GEOM_ROWS);
    SGS_HIP(ctx, hipMemcpy(rows.data(), sc->geom.p, rows.size() * sizeof(float4), hipMemcpyDeviceToHost));
    float* dst = (float*)host_dst;
    for (int64_t p = 0; p < sc->n; ++p) {
        const int64_t chunk = p >> 6, lane = p & 63;
        const float4 g0 = rows[(size_t)((chunk * SGS_GEOM_ROWS + 0) * 64 + lane)], g1 = rows[(size_t)((chunk * SGS_GEOM_ROWS + 1) * 64 + lane)],
                     g2 = rows[(size_t)((chunk * SGS_GEOM_ROWS + 2) * 64 + lane)];
        unsigned i; memcpy(&i, &g2.w, 4);
        if ((int64_t)(i + 1) * 11 * 4 > n) continue;
        float* o = dst + (size_t)i * 11;
        o[0] = g0.x; o[1] = g0.y; o[2] = g0.z; o[3] = g0.w; o[4] = g1.x; o[5] = g1.y; o[6] = g1.z; o[7] = g1.w; o[8] = g2.x; o[9] = g2.y; o[10] = g2.z;
    }
    return SGS_OK;
}

// the scene's SH coefficients as k_preprocess evaluates them, back in the caller's order: [N, K, 3] fp32
int read_scene_sh(sgs_ctx* ctx, const sgs_scene* sc, int64_t n_slots, void* host_dst, int64_t n) {
    const int nf = 3 * (sc->sh_degree + 1) * (sc->sh_degree + 1), rows_n = sc->sh_rows;
    std::vector<float4> rows((size_t)n_slots * rows_n), geo((size_t)n_slots * SGS_GEOM_ROWS);
    SGS_HIP(ctx, hipMemcpy(rows.data(), sc->shq.p, rows.size() * sizeof(float4), hipMemcpyDeviceToHost));
    SGS_HIP(ctx, hipMemcpy(geo.data(), sc->geom.p, geo.size() * sizeof(float4), hipMemcpyDeviceToHost));
    float* dst = (float*)host_dst;
    std::vector<unsigned> w((size_t)rows_n * 4);
    for (int64_t p = 0; p < sc->n; ++p) {
        const int64_t chunk = p >> 6, lane = p & 63;
        unsigned i; memcpy(&i, &geo[(size_t)((chunk * SGS_GEOM_ROWS + 2) * 64 + lane)].w, 4);       // the original index
        if ((int64_t)(i + 1) * nf * 4 > n) continue;
        for (int r = 0; r < rows_n; ++r) memcpy(&w[(size_t)4 * r], &rows[(size_t)((chunk * rows_n + r) * 64 + lane)], 16);
        float* o = dst + (size_t)i * nf;
        if (!sc->sh_packed) memcpy(o, w.data(), (size_t)nf * 4);
        else {      // 12 B of fp32 DC, then a byte per coefficient: v / 32 - 4 + 1 / 64, exact in fp32 (sgs_kernels.h sgs_sh_byte)
            memcpy(o, w.data(), 12);
            for (int j = 0; j < nf - 3; ++j) {      // sgs_kernels.h sgs_sh_byte / sgs_sh_byte_mode, restated: one correctly rounded fma (exact in double, rounded once)
                const unsigned v = (w[(size_t)3 + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
                volatile double prod = (double)v * (8.0 / 255.0);         // (two roundings, as the kernel's __dmul_rn / __dsub_rn)
                float x = sc->sh_decode == 1 ? (float)(prod - 4.0) : (float)((double)v * (1.0 / 32.0) + (-4.0 + 1.0 / 64.0));
                if (sc->sh_decode == 2) x = v == 0u ? -4.0f : v == 255u ? 4.0f : x;
                o[3 + j] = x;
            }
        }
    }
    return SGS_OK;
}

// per chunk: 1 = the per-chunk bounds skipped it (no slot live, every slot "big": k_chunk_cull's mark)
int read_chunk_skipped(sgs_ctx* ctx, const Lane& L, int64_t n_chunks, void* host_dst, int64_t n) {
    std::vector<unsigned long long> vm((size_t)std::max<int64_t>(1, n_chunks)), bm(vm.size());
    SGS_HIP(ctx, hipMemcpy(vm.data(), L.vismask.p, (size_t)n_chunks * 8, hipMemcpyDeviceToHost));
    SGS_HIP(ctx, hipMemcpy(bm.data(), L.bigmask.p, (size_t)n_chunks * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) ((unsigned char*)host_dst)[i] = vm[(size_t)i] == 0ull && bm[(size_t)i] == ~0ull;
    return SGS_OK;
}

// device records (sgs_common.h: 64 B, conic pre-scaled for the composite, opacity also as an exponent offset) -> x,y,conic a,b | c,opacity,r,g | b,depth,rect01,rect23
// The device holds a record at its Gaussian's LAYOUT position; the caller gets it at the ORIGINAL index (perm: layout position -> original
// index, nullptr = identity; the padding of the last chunk lies behind both orders).
int read_splats(sgs_ctx* ctx, const FrameRec& r, const Lane& L, void* host_dst, int64_t n, int64_t elem) {
    const int64_t cnt = n / elem, n_slots = (r.n + 63) / 64 * 64;
    const unsigned* perm = r.scene && !r.scene->perm_host.empty() ? r.scene->perm_host.data() : nullptr;
    const int64_t n_read = perm ? n_slots : cnt;           // (a short read of a permuted scene may want any of the records)
    std::vector<Splat> tmp((size_t)std::max<int64_t>(1, n_read));
    SGS_HIP(ctx, hipMemcpy(tmp.data(), L.splats.p, (size_t)n_read * sizeof(Splat), hipMemcpyDeviceToHost));
    const double l2e = 1.4426950408889634;
    for (int64_t p = 0; p < n_read; ++p) {
        const int64_t i = perm && p < r.n ? (int64_t)perm[(size_t)p] : p;
        if (i >= cnt) continue;
        const Splat& sp = tmp[(size_t)p];
        float* o = (float*)((char*)host_dst + i * elem);
        o[0] = sp.x; o[1] = sp.y;
        // (the record holds the roots of the completed square A (dx + k dy)^2 + C' dy^2 in the slots A, B, C: a = sqrt(A),
        //  a k, c = +-sqrt(|C'|);  B = 2 A k = 2 a (a k),  C = A k^2 + C' = (a k)^2 + C')
        const double a_ = sp.A, ak_ = sp.B, c_ = sp.C;
        const double A_ = a_ * a_, Cp_ = c_ * std::fabs(c_);
        o[2] = (float)(A_ / (0.5 * l2e)); o[3] = (float)(2.0 * a_ * ak_ / l2e); o[4] = (float)((ak_ * ak_ + Cp_) / (0.5 * l2e));
        o[5] = sp.o; o[6] = sp.r; o[7] = sp.g; o[8] = sp.b;
        memcpy(o + 9, &sp.key, 4); memcpy(o + 10, &sp.rect01, 4); memcpy(o + 11, &sp.rect23, 4);
    }
    return SGS_OK;
}

// The caller sees a splat at its Gaussian's index (read_splats); the per-chunk visibility masks, by layout position, say which are live.
// Dead slots are blanked (slot ids -> 0xFFFFFFFF, splats -> 0) so stale data cannot pass for live.
int blank_dead_slots(sgs_ctx* ctx, const FrameRec& r, const Lane& L, bool slot_ids, void* host_dst, int64_t n, int64_t elem) {
    const int64_t n_chunks = (r.n + 63) / 64, n_slots = n_chunks * 64;
    std::vector<unsigned long long> vm((size_t)std::max<int64_t>(1, n_chunks));
    SGS_HIP(ctx, hipMemcpy(vm.data(), L.vismask.p, (size_t)n_chunks * 8, hipMemcpyDeviceToHost));
    char* dst = (char*)host_dst;
    // vismask is indexed by layout position; slots by original index
    const unsigned* perm = r.scene && !r.scene->perm_host.empty() ? r.scene->perm_host.data() : nullptr;
    std::vector<unsigned char> live((size_t)n_slots, 0);
    for (int64_t p = 0; p < r.n; ++p)
        if ((vm[p >> 6] >> (p & 63)) & 1ull) live[perm ? perm[p] : (size_t)p] = 1;
    for (int64_t i = 0; i < n_slots && (i + 1) * elem <= n; ++i) {
        if (slot_ids) ((unsigned*)dst)[i] = live[(size_t)i] ? (unsigned)i : 0xFFFFFFFFu;
        else if (!live[(size_t)i]) memset(dst + i * elem, 0, (size_t)elem);
    }
    return SGS_OK;
}

}  // namespace

int64_t sgs_debug_read(sgs_ctx* ctx, int what, void* host_dst, int64_t bytes) {
    if (!ctx) return SGS_ERR_INVALID;
    const FrameRec& r = ctx->last;
    if (r.slot < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "no frame has been rendered");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    SGS_HIP(ctx, hipDeviceSynchronize());
    const FrameStatus& s = ctx->ring.h_status.p[r.slot];
    const Lane& L = ctx->lanes[r.lane];
    const sgs_scene* sc = r.scene;
    const int64_t n_chunks = (r.n + 63) / 64;
    const int64_t n_slots = n_chunks * 64;
    // (a growth that failed since that frame has emptied what it was replacing)
    if (!L.splats.holds(n_slots) || !L.vismask.holds(n_chunks) || !L.bigmask.holds(n_chunks) || !L.tile_offset.holds((int64_t)r.T + 1))
        SGS_FAIL(ctx, SGS_ERR_INVALID, "the last frame's intermediates are gone: an allocation has failed since");
    const void* src = nullptr;
    int64_t have = 0, elem = 0;
    switch (what) {
        case SGS_BUF_TILE_OFFSETS: have = ((int64_t)r.T + 1) * 4; break;       // every 8th sub-queue offset
        case SGS_BUF_SORTED_SLOTS: src = L.sorted_out.p; have = (s.overflow || !L.sorted_out.p) ? 0 : (int64_t)s.d_total * 4; break;
        case SGS_BUF_SLOT_IDS: elem = 4; have = n_slots * elem; break;
        case SGS_BUF_SPLATS: elem = 48; have = n_slots * elem; break;          // the 12-word view documented in sage_gs.h
        case SGS_BUF_CHUNK_SKIPPED: have = n_chunks; break;
        case SGS_BUF_SCENE_GEOM: have = sc ? r.n * 11 * 4 : 0; break;
        case SGS_BUF_SCENE_SH: have = sc ? r.n * 3 * (sc->sh_degree + 1) * (sc->sh_degree + 1) * 4 : 0; break;
        case SGS_BUF_SCENE_PERM: have = sc ? r.n * 4 : 0; break;
        case SGS_BUF_CHUNK_BOUNDS: src = sc ? sc->cbound.p : nullptr; have = src ? n_chunks * 32 : 0; break;
        case 100: src = L.tile_prof.p; have = (int64_t)r.T * 8 * SGS_PROF_WORDS; break;    // profiling build only
        case 101: src = L.bin_prof.p; have = (int64_t)SGS_BIN_BLOCKS * 64; break;  // profiling build only
        default: SGS_FAIL(ctx, SGS_ERR_INVALID, "unknown buffer id %d", what);
    }
    const int64_t n = std::min(have, bytes);
    if (n <= 0 || !host_dst) return have;
    int rc = SGS_OK;
    if (src) SGS_HIP(ctx, hipMemcpy(host_dst, src, (size_t)n, hipMemcpyDeviceToHost));
    if (what == SGS_BUF_TILE_OFFSETS) rc = read_tile_offsets(ctx, r, L, host_dst, n);
    if (what == SGS_BUF_SCENE_PERM) {      // the host copy layout_scene kept (empty: the scene is in the caller's order)
        const std::vector<unsigned>& perm = sc->perm_host;
        for (int64_t p = 0; (p + 1) * 4 <= n; ++p) ((unsigned*)host_dst)[p] = perm.empty() ? (unsigned)p : perm[(size_t)p];
    }
    if (what == SGS_BUF_SCENE_GEOM) rc = read_scene_geom(ctx, sc, n_slots, host_dst, n);
    if (what == SGS_BUF_SCENE_SH) rc = read_scene_sh(ctx, sc, n_slots, host_dst, n);
    if (what == SGS_BUF_CHUNK_SKIPPED) rc = read_chunk_skipped(ctx, L, n_chunks, host_dst, n);
    if (what == SGS_BUF_SPLATS) rc = read_splats(ctx, r, L, host_dst, n, elem);
    if (rc == SGS_OK && elem) rc = blank_dead_slots(ctx, r, L, what == SGS_BUF_SLOT_IDS, host_dst, n, elem);
    return rc != SGS_OK ? rc : have;
}

// ---- collision-mesh depth (include/sage_gs.h "Collision-mesh depth"; kernels in sgs_mesh.h) ------------------------------------------

int sgs_mesh_upload(sgs_ctx* ctx, int64_t n_vertices, const float* vertices, int64_t n_triangles, const int32_t* triangles,
                    int on_device, sgs_mesh** out) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!out) SGS_FAIL(ctx, SGS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_vertices < 0 || n_vertices > 0x7fffffffll) SGS_FAIL(ctx, SGS_ERR_INVALID, "n_vertices = %lld out of range", (long long)n_vertices);
    if (n_triangles < 0 || n_triangles > (1ll << 28)) SGS_FAIL(ctx, SGS_ERR_INVALID, "n_triangles = %lld out of range [0, 2^28]", (long long)n_triangles);
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) SGS_FAIL(ctx, SGS_ERR_INVALID, "null input array");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    MeshScratch& M = ctx->mesh;
    int rc;
    if ((rc = ensure_mesh_status(ctx)) != SGS_OK) return rc;
    std::unique_ptr<sgs_mesh> m(new (std::nothrow) sgs_mesh);      // (released with its buffers by any return before *out)
    if (!m) SGS_FAIL(ctx, SGS_ERR_OOM, "out of host memory");
    m->n_verts = n_vertices; m->n_tris = n_triangles;
    const size_t vb = (size_t)n_vertices * 12, tb = (size_t)n_triangles * 12;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    SGS_HIP(ctx, m->verts.grow(std::max<int64_t>(3 * n_vertices, 4)));
    SGS_HIP(ctx, m->tris.grow(std::max<int64_t>(3 * n_triangles, 4)));
    if (vb) SGS_HIP(ctx, hipMemcpy(m->verts.p, vertices, vb, kind));
    if (tb) SGS_HIP(ctx, hipMemcpy(m->tris.p, triangles, tb, kind));
    // the checks run on the device (the caller's arrays may live there): a status word, read back once
    unsigned* bad = &M.d_st.p[SGS_MESH_MAX_GROUP].n_visible;
    SGS_HIP(ctx, hipMemset(bad, 0, sizeof(unsigned)));
    const long long work = 3 * std::max<long long>(n_vertices, n_triangles);
    const float* const d_verts = m->verts.p;
    const int* const d_tris = m->tris.p;
    if (work > 0)
        hipLaunchKernelGGL(sgs::k_mesh_validate, dim3((unsigned)std::min<long long>((work + 255) / 256, 4096)), dim3(256), 0, nullptr,
                           (long long)n_vertices, d_verts, (long long)n_triangles, d_tris, bad);
    unsigned flags = 0;
    SGS_HIP(ctx, hipGetLastError());
    SGS_HIP(ctx, hipMemcpy(&flags, bad, sizeof flags, hipMemcpyDeviceToHost));
    if (flags)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh upload: %s%s", (flags & 1u) ? "non-finite vertex coordinates " : "",
                 (flags & 2u) ? "triangle indices outside [0, n_vertices)" : "");
    *out = m.release();
    return SGS_OK;
}

int sgs_mesh_free(sgs_ctx* ctx, sgs_mesh* mesh) {
    if (!mesh) return SGS_OK;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipDeviceSynchronize(); }
    delete mesh;
    return SGS_OK;
}

int sgs_mesh_set_labels(sgs_ctx* ctx, sgs_mesh* mesh, const int32_t* labels, int on_device) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!mesh) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh is NULL");
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    SGS_HIP(ctx, hipDeviceSynchronize());                    // no frame still reads the labels that are replaced
    DevBuf<int> fresh;                                       // (the mesh keeps its previous labels unless these pass)
    if (labels && mesh->n_tris > 0) {
        SGS_HIP(ctx, fresh.grow(mesh->n_tris));
        SGS_HIP(ctx, hipMemcpy(fresh.p, labels, (size_t)mesh->n_tris * sizeof(int), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        // checked on the device (the caller's array may live there), through the upload's status word
        if (!ctx->mesh.d_st.p) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh labels: the mesh was not uploaded through this context");
        unsigned* bad = &ctx->mesh.d_st.p[SGS_MESH_MAX_GROUP].n_visible;
        unsigned flags = 0;
        SGS_HIP(ctx, hipMemset(bad, 0, sizeof(unsigned)));
        const int* const d_labels = fresh.p;
        hipLaunchKernelGGL(sgs::k_mesh_validate_labels, dim3((unsigned)std::min<long long>((mesh->n_tris + 255) / 256, 4096)), dim3(256), 0,
                           nullptr, (long long)mesh->n_tris, d_labels, bad);
        SGS_HIP(ctx, hipGetLastError());
        SGS_HIP(ctx, hipMemcpy(&flags, bad, sizeof flags, hipMemcpyDeviceToHost));
        if (flags) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh labels: labels outside [0, INT32_MAX - 1] (the mesh keeps its previous labels)");
    }
    mesh->labels = std::move(fresh);
    return SGS_OK;
}

int sgs_mesh_set_record_capacity(sgs_ctx* ctx, int64_t max_records) {
    if (!ctx) return SGS_ERR_INVALID;
    if (max_records < 1 || max_records > kMaxRecords) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh record capacity %lld outside [1, 2^32)", (long long)max_records);
    MeshScratch& M = ctx->mesh;
    M.cap_wanted = max_records;
    if (M.list.p && M.list.cap != max_records) {             // reallocated at the requested size by the next mesh frame
        SGS_HIP(ctx, hipSetDevice(ctx->device));
        SGS_HIP(ctx, hipDeviceSynchronize());
        M.list.reset();
    }
    return SGS_OK;
}

}  // extern "C"

namespace {

// Frames [0, n) of cams: groups of up to SGS_MESH_MAX_GROUP frames, each five launches and one synchronisation; frame i is written at
// out + i * frame_stride.  stats: n entries (nullable).  out_id != nullptr: the id frames (sgs_render_mesh_ids*: k_mesh_ids as the last
// launch, out nullable); otherwise the depth frames.
int mesh_frames(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cams, int n, const sgs_config* cfg_in, int row_begin, int row_end,
                float* out, int32_t* out_id, bool ids, int64_t frame_stride, sgs_stats* stats, void* hip_stream) {
    if (!mesh || !cams || (ids ? !out_id : !out)) SGS_FAIL(ctx, SGS_ERR_INVALID, "null mesh / camera / output");
    if (n < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "n_cams = %d", n);
    sgs_config cfg;
    if (cfg_in) cfg = *cfg_in; else sgs_config_default(&cfg);
    if (cfg.tile_row_stride > 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh depth: interleaved tile rows (tile_row_stride %d) are not supported", cfg.tile_row_stride);
    if (cfg.flags & (SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED)) SGS_FAIL(ctx, SGS_ERR_INVALID, "mesh depth is synchronous only: SGS_FLAG_ASYNC / SGS_FLAG_PIPELINED are refused");
    if (!(cfg.near_z > 0.f) || !(cfg.far_z > cfg.near_z)) SGS_FAIL(ctx, SGS_ERR_INVALID, "need 0 < near_z < far_z (got %g, %g)", cfg.near_z, cfg.far_z);
    const int W = cams[0].width, H = cams[0].height;
    for (int i = 0; i < n; ++i) {
        const sgs_camera* c = &cams[i];
        if (c->width != W || c->height != H) SGS_FAIL(ctx, SGS_ERR_INVALID, "camera %d: %dx%d, camera 0: %dx%d (one resolution per call)", i, c->width, c->height, W, H);
        if (!std::isfinite(c->cx) || !std::isfinite(c->cy)) SGS_FAIL(ctx, SGS_ERR_INVALID, "principal point must be finite");
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(c->view[k])) SGS_FAIL(ctx, SGS_ERR_INVALID, "camera %d: non-finite view", i);
        char why[160];
        if (check_camera(*c, why, sizeof why)) SGS_FAIL(ctx, SGS_ERR_INVALID, "camera %d: %s", i, why);
    }
    const int gy = (H + SGS_TILE - 1) / SGS_TILE, gx = (W + SGS_TILE - 1) / SGS_TILE;
    if (row_end < 0 || row_end > gy) row_end = gy;
    if (row_begin < 0) row_begin = 0;
    if (row_begin > row_end) SGS_FAIL(ctx, SGS_ERR_INVALID, "tile_row_begin %d > tile_row_end %d", row_begin, row_end);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    MeshScratch& M = ctx->mesh;
    int rc;
    if ((rc = ensure_mesh_status(ctx)) != SGS_OK) return rc;
    const bool timed = (cfg.flags & SGS_FLAG_TIMING) != 0;
    if (timed) { SGS_HIP(ctx, M.ev[0].create()); SGS_HIP(ctx, M.ev[1].create()); }
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int n_tiles = (row_end - row_begin) * gx;
    const int64_t F = mesh->n_tris;
    for (int g0 = 0; g0 < n; g0 += SGS_MESH_MAX_GROUP) {
        const int nf = std::min(SGS_MESH_MAX_GROUP, n - g0);
        const int64_t slots = std::max<int64_t>(F * nf, 1), tiles = (int64_t)n_tiles * nf + nf;
        SGS_HIP(ctx, M.rec.grow(4 * slots));
        SGS_HIP(ctx, M.rect.grow(slots));
        SGS_HIP(ctx, M.big.grow(slots));
        SGS_HIP(ctx, M.counts.grow(tiles));
        SGS_HIP(ctx, M.offs.grow(tiles));
        int retries = 0;
        for (;;) {
            SGS_HIP(ctx, M.list.grow(M.cap_wanted));
            sgs::MeshGroup G;
            memset(&G, 0, sizeof G);
            for (int f = 0; f < nf; ++f) {
                const sgs_camera& c = cams[g0 + f];
                sgs::MeshFrame& P = G.f[f];
                for (int k = 0; k < 12; ++k) P.view[k] = c.view[k];
                P.fx = c.fx; P.fy = c.fy; P.cx = c.cx; P.cy = c.cy; P.near_z = cfg.near_z; P.far_z = cfg.far_z;
                P.width = W; P.height = H; P.gx = gx; P.row_begin = row_begin; P.row_end = row_end;
                P.out = out ? out + (int64_t)(g0 + f) * frame_stride : nullptr;
                P.out_id = ids ? out_id + (int64_t)(g0 + f) * frame_stride : nullptr;
            }
            G.nf = nf; G.n_tiles = n_tiles; G.n_tris = F; G.cap = M.list.cap;
            G.verts = mesh->verts.p; G.tris = mesh->tris.p; G.labels = mesh->labels.p;
            G.rec = M.rec.p; G.rect = M.rect.p; G.big = M.big.p; G.counts = M.counts.p; G.offs = M.offs.p; G.list = M.list.p; G.st = M.d_st.p;
            if (timed) SGS_HIP(ctx, hipEventRecord(M.ev[0].e, stream));
            SGS_HIP(ctx, hipMemsetAsync(M.d_st.p, 0, sizeof(sgs::MeshStatus) * nf, stream));
            if (n_tiles > 0) {
                SGS_HIP(ctx, hipMemsetAsync(M.counts.p, 0, sizeof(unsigned) * (size_t)n_tiles * nf, stream));
                if (F > 0) {
                    hipLaunchKernelGGL(sgs::k_mesh_setup, dim3((unsigned)((F + 255) / 256), (unsigned)nf), dim3(256), 0, stream, G);
                    const unsigned bin_grid = (unsigned)std::min<int64_t>((F + 255) / 256, SGS_MESH_BIN_BLOCKS);
                    hipLaunchKernelGGL(sgs::k_mesh_bin<false>, dim3(bin_grid, (unsigned)nf), dim3(256), 0, stream, G);
                    hipLaunchKernelGGL(sgs::k_mesh_scan, dim3(1, (unsigned)nf), dim3(SGS_MESH_SCAN_THREADS), 0, stream, G);
                    hipLaunchKernelGGL(sgs::k_mesh_bin<true>, dim3(bin_grid, (unsigned)nf), dim3(256), 0, stream, G);
                } else {
                    hipLaunchKernelGGL(sgs::k_mesh_scan, dim3(1, (unsigned)nf), dim3(SGS_MESH_SCAN_THREADS), 0, stream, G);
                }
                if (ids) hipLaunchKernelGGL(sgs::k_mesh_ids, dim3((unsigned)n_tiles, (unsigned)nf), dim3(256), 0, stream, G);
                else hipLaunchKernelGGL(sgs::k_mesh_depth, dim3((unsigned)n_tiles, (unsigned)nf), dim3(256), 0, stream, G);
            }
            if (timed) SGS_HIP(ctx, hipEventRecord(M.ev[1].e, stream));
            SGS_HIP(ctx, hipGetLastError());
            SGS_HIP(ctx, hipMemcpyAsync(M.h_st.p, M.d_st.p, sizeof(sgs::MeshStatus) * nf, hipMemcpyDeviceToHost, stream));
            SGS_HIP(ctx, hipStreamSynchronize(stream));
            int64_t total = 0;
            for (int f = 0; f < nf; ++f) total += M.h_st.p[f].d_total;
            if (total <= M.list.cap) {
                float ms = 0.f;
                if (timed) SGS_HIP(ctx, hipEventElapsedTime(&ms, M.ev[0].e, M.ev[1].e));
                for (int f = 0; f < nf && stats; ++f) {
                    sgs_stats& s = stats[g0 + f];
                    memset(&s, 0, sizeof s);
                    s.n_visible = M.h_st.p[f].n_visible;
                    s.d_total = M.h_st.p[f].d_total;
                    s.max_tile_len = (int32_t)M.h_st.p[f].max_tile_len;
                    s.n_tiles = n_tiles;
                    s.n_pixels = (int64_t)W * (std::min(H, SGS_TILE * row_end) - SGS_TILE * row_begin);
                    s.retries = retries;
                    s.ms_total = ms / (float)nf;
                }
                break;
            }
            // the record buffer overflowed: grow it to fit and render the group again
            if (++retries > 4) SGS_FAIL(ctx, SGS_ERR_OVERFLOW, "mesh record buffer still too small after 4 retries");
            M.cap_wanted = std::min<int64_t>(std::max<int64_t>(total + total / 4, M.list.cap * 2), kMaxRecords);
            if (total > kMaxRecords) SGS_FAIL(ctx, SGS_ERR_OVERFLOW, "mesh depth: %lld records exceed 2^32", (long long)total);
        }
    }
    return SGS_OK;
}

}  // namespace

extern "C" {

int sgs_render_mesh_depth(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cam, const sgs_config* cfg, int tile_row_begin,
                          int tile_row_end, float* out_depth, sgs_stats* stats, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    return mesh_frames(ctx, mesh, cam, 1, cfg, tile_row_begin, tile_row_end, out_depth, nullptr, false, 0, stats, hip_stream);
}

int sgs_render_mesh_depth_batch(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cams, int n_cams, const sgs_config* cfg,
                                float* out_depth, sgs_stats* stats, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!cams || n_cams < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "no cameras");
    return mesh_frames(ctx, mesh, cams, n_cams, cfg, 0, -1, out_depth, nullptr, false, (int64_t)cams[0].width * cams[0].height, stats, hip_stream);
}

int sgs_render_mesh_ids(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cam, const sgs_config* cfg, int tile_row_begin,
                        int tile_row_end, float* out_depth, int32_t* out_id, sgs_stats* stats, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    return mesh_frames(ctx, mesh, cam, 1, cfg, tile_row_begin, tile_row_end, out_depth, out_id, true, 0, stats, hip_stream);
}

int sgs_render_mesh_ids_batch(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cams, int n_cams, const sgs_config* cfg,
                              float* out_depth, int32_t* out_id, sgs_stats* stats, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    if (!cams || n_cams < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "no cameras");
    return mesh_frames(ctx, mesh, cams, n_cams, cfg, 0, -1, out_depth, out_id, true, (int64_t)cams[0].width * cams[0].height, stats, hip_stream);
}

}  // extern "C"

// ---- the file encoders: what they share on the host (csrc/sgs_encode.h is the device side) ------------------------------------------
namespace {

// The checks every encoder makes of its arguments, after its own of the picture's parameters (bad_params: what is wrong with those, or
// nullptr).  src_name: what the entry point calls its input; units: what a frame is cut into.
int check_file_args(sgs_ctx* ctx, const char* who, const char* bad_params, int n_frames, const float* src, const char* src_name, int64_t frame_stride,
                    int64_t frame_floats, const uint8_t* out, int64_t out_capacity, const int64_t* out_offsets, const int64_t* out_sizes,
                    int units_per_frame, const char* units) {
    if (!ctx) return SGS_ERR_INVALID;
    if (bad_params) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %s", who, bad_params);
    if (n_frames < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    if (!src) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: null %s", who, src_name);
    if (!out) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: null out", who);
    if (!out_offsets) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: null out_offsets", who);
    if (!out_sizes) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: null out_sizes", who);
    if (out_capacity < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: out_capacity %lld is negative", who, (long long)out_capacity);
    if (n_frames > 1 && frame_stride < frame_floats)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: frames overlap (stride %lld floats, a frame has %lld)", who, (long long)frame_stride, (long long)frame_floats);
    const int64_t n = (int64_t)n_frames * units_per_frame;
    if (n > 0x7fffffffll) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %lld %s in one call (at most 2^31 - 1)", who, (long long)n, units);
    return SGS_OK;
}

// Readies K for a call of n_units units: the pinned status words (made on first use) and the offsets array.  A call of no frames has
// nothing to place: the status becomes this call's, not the previous one's, and K is left alone.
int ready_file_sink(sgs_ctx* ctx, FileScratch& F, int64_t n_units, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* out_sizes,
                    sgs::FileSink& K) {
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    if (!F.h_status.p) {
        SGS_HIP(ctx, F.h_status.grow(2));
        F.h_status.p[0] = F.h_status.p[1] = 0;
    }
    if (n_units == 0) {
        F.h_status.p[0] = 0; F.h_status.p[1] = out_capacity;
        return SGS_OK;
    }
    // (the scratch arrays of the encoders and the resize grow geometrically; releasing the old array waits for the work that still uses it)
    SGS_HIP(ctx, F.offs.grow(n_units + 1, Grow::geometric));
    K = {F.offs.p, out, out_capacity, reinterpret_cast<long long*>(out_offsets), reinterpret_cast<long long*>(out_sizes), F.h_status.p};
    return SGS_OK;
}

// sgs_jpeg_status / sgs_png_status: the status words of the encoder's most recent call (F: nullptr without a context).
int file_status(sgs_ctx* ctx, const char* who, const FileScratch* F, int64_t* bytes_needed) {
    if (!ctx) return SGS_ERR_INVALID;
    const long long need = F->h_status.p ? F->h_status.p[0] : 0, cap = F->h_status.p ? F->h_status.p[1] : 0;
    if (bytes_needed) *bytes_needed = need;
    if (need > cap) SGS_FAIL(ctx, SGS_ERR_OVERFLOW, "%s: the files take %lld bytes, out_capacity was %lld", who, need, cap);
    return SGS_OK;
}

// ---- JPEG encoder (csrc/sgs_jpeg.h) ------------------------------------------------------------------------------------------------
struct JpegGeom { int s420, mcus_x, mcus_y, n_mcu, ri, n_int; };

// nullptr when the arguments describe a picture the encoder takes, else what is wrong with them.
const char* jpeg_geom(int width, int height, const sgs_jpeg_params* p, JpegGeom& g, char* why, size_t n_why) {
    if (!p) { snprintf(why, n_why, "params is NULL"); return why; }
    if (p->quality < 1 || p->quality > 100) { snprintf(why, n_why, "quality %d is outside 1..100", p->quality); return why; }
    if (p->subsampling != SGS_JPEG_420 && p->subsampling != SGS_JPEG_444) {
        snprintf(why, n_why, "subsampling %d is neither SGS_JPEG_420 nor SGS_JPEG_444", p->subsampling); return why;
    }
    if (width < 1 || height < 1 || width > 65535 || height > 65535) { snprintf(why, n_why, "%d x %d is outside 1..65535", width, height); return why; }
    g.s420 = p->subsampling == SGS_JPEG_420;
    const int mcu = g.s420 ? 16 : 8;
    g.mcus_x = (width + mcu - 1) / mcu; g.mcus_y = (height + mcu - 1) / mcu;
    g.n_mcu = g.mcus_x * g.mcus_y;
    g.ri = SGS_JPEG_BLOCKS / (g.s420 ? 6 : 3);
    g.n_int = (g.n_mcu + g.ri - 1) / g.ri;
    return nullptr;
}

}  // namespace

extern "C" {

void sgs_jpeg_params_default(sgs_jpeg_params* p) {
    if (!p) return;
    p->quality = 95; p->subsampling = SGS_JPEG_420; p->flags = 0; p->reserved_ = 0;
}

int64_t sgs_jpeg_bound(int width, int height, const sgs_jpeg_params* params) {
    JpegGeom g;
    char why[256];
    if (jpeg_geom(width, height, params, g, why, sizeof why)) return SGS_ERR_INVALID;
    return SGS_JPEG_HEADER + (int64_t)g.n_int * (2 * SGS_JPEG_INT_BYTES + 2);
}

int sgs_encode_jpeg(sgs_ctx* ctx, const float* rgb, int width, int height, int n_frames, int64_t rgb_frame_stride,
                    const sgs_jpeg_params* params, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* out_sizes,
                    void* hip_stream) {
    JpegGeom g = {};
    char why[256];
    const char* bad = jpeg_geom(width, height, params, g, why, sizeof why);
    int rc = check_file_args(ctx, "sgs_encode_jpeg", bad, n_frames, rgb, "rgb", rgb_frame_stride, (int64_t)width * height * 3, out, out_capacity,
                             out_offsets, out_sizes, g.n_int, "restart intervals");
    if (rc != SGS_OK) return rc;
    const int64_t n = (int64_t)n_frames * g.n_int;
    JpegScratch& Z = ctx->jpeg;
    sgs::JpegJob J;
    if ((rc = ready_file_sink(ctx, Z.files, n, out, out_capacity, out_offsets, out_sizes, J.sink)) != SGS_OK || n == 0) return rc;
    sgs::JpegTables* tab = nullptr;
    for (const JpegScratch::Entry& e : Z.tables)
        if (e.width == width && e.height == height && e.quality == params->quality && e.s420 == g.s420) tab = e.dev.p;
    if (!tab) {
        sgs::JpegTables T;
        memset(&T, 0, sizeof T);
        sgs::jpeg::build_tables(T, width, height, params->quality, g.s420 != 0, g.ri);
        DevBuf<sgs::JpegTables> fresh;
        SGS_HIP(ctx, fresh.grow(1));
        SGS_HIP(ctx, hipMemcpy(fresh.p, &T, sizeof T, hipMemcpyHostToDevice));         // (synchronous: T is on this stack)
        tab = fresh.p;
        // only a filled table is remembered.  The list is never trimmed: 4.3 KB of device memory per distinct (width, height, quality,
        // subsampling) a context has encoded, until sgs_destroy — a handful in any real caller
        Z.tables.push_back({width, height, params->quality, g.s420, std::move(fresh)});
    }
    SGS_HIP(ctx, Z.sizes.grow(n, Grow::geometric));
    J.rgb = rgb; J.frame_stride = rgb_frame_stride; J.width = width; J.height = height; J.s420 = g.s420;
    J.mcus_x = g.mcus_x; J.n_mcu = g.n_mcu; J.ri = g.ri; J.n_int = g.n_int; J.n_frames = n_frames;
    J.tab = tab; J.sizes = Z.sizes.p;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(sgs::k_jpeg_intervals<false>, dim3((unsigned)n), dim3(64), 0, st, J);
    hipLaunchKernelGGL(sgs::k_jpeg_scan, dim3(1), dim3(SGS_JPEG_SCAN_THREADS), 0, st, J);
    hipLaunchKernelGGL(sgs::k_jpeg_intervals<true>, dim3((unsigned)n), dim3(64), 0, st, J);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

int sgs_jpeg_status(sgs_ctx* ctx, int64_t* bytes_needed) {
    return file_status(ctx, "sgs_encode_jpeg", ctx ? &ctx->jpeg.files : nullptr, bytes_needed);
}

}  // extern "C"

// ---- PNG encoder (csrc/sgs_png.h) -------------------------------------------------------------------------------------------------
namespace {

struct PngGeom { int depth16, bpp, row_bytes, rows_per_strip, n_strips; };

// nullptr when the arguments describe a picture the encoder takes, else what is wrong with them.
const char* png_geom(int width, int height, const sgs_png_params* p, PngGeom& g, char* why, size_t n_why) {
    if (!p) { snprintf(why, n_why, "params is NULL"); return why; }
    if (p->format != SGS_PNG_RGB8 && p->format != SGS_PNG_DEPTH16) {
        snprintf(why, n_why, "format %d is neither SGS_PNG_RGB8 nor SGS_PNG_DEPTH16", p->format); return why;
    }
    if (p->reserved != 0) { snprintf(why, n_why, "reserved = %d, must be 0", p->reserved); return why; }
    if (width < 1 || height < 1 || height > 65535) { snprintf(why, n_why, "%d x %d: width < 1 or height outside 1..65535", width, height); return why; }
    g.depth16 = p->format == SGS_PNG_DEPTH16;
    g.bpp = g.depth16 ? 2 : 3;
    if ((int64_t)width * g.bpp + 1 > SGS_PNG_STRIP) {
        snprintf(why, n_why, "width %d: a filtered row of %lld bytes is longer than %d", width, (long long)width * g.bpp + 1, SGS_PNG_STRIP); return why;
    }
    if (g.depth16) {
        if (!(p->depth_scale > 0.f)) { snprintf(why, n_why, "depth_scale %g is not positive", (double)p->depth_scale); return why; }
        if (!(p->depth_max > 0.f)) { snprintf(why, n_why, "depth_max %g is not positive", (double)p->depth_max); return why; }
        const volatile float top = p->depth_max * p->depth_scale;              // the kernel's own fp32 product of the largest clamped depth
        if (!(top <= 65535.0f)) {
            snprintf(why, n_why, "depth_max * depth_scale = %.9g does not fit 16 bits", (double)top); return why;
        }
    }
    g.row_bytes = width * g.bpp;
    g.rows_per_strip = std::max(1, SGS_PNG_STRIP / (g.row_bytes + 1));
    g.n_strips = (height + g.rows_per_strip - 1) / g.rows_per_strip;
    return nullptr;
}

}  // namespace

extern "C" {

void sgs_png_params_default(sgs_png_params* p) {
    if (!p) return;
    p->format = SGS_PNG_RGB8; p->depth_scale = 10000.0f; p->depth_max = 6.5f; p->reserved = 0;
}

int64_t sgs_png_bound(int width, int height, const sgs_png_params* params) {
    PngGeom g;
    char why[256];
    if (png_geom(width, height, params, g, why, sizeof why)) return SGS_ERR_INVALID;
    return 56 + (int64_t)g.n_strips * 22 + (int64_t)height * (g.row_bytes + 1);
}

int sgs_encode_png(sgs_ctx* ctx, const float* src, int width, int height, int n_frames, int64_t src_frame_stride,
                   const sgs_png_params* params, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* out_sizes,
                   void* hip_stream) {
    PngGeom g = {};
    char why[256];
    const char* bad = png_geom(width, height, params, g, why, sizeof why);
    int rc = check_file_args(ctx, "sgs_encode_png", bad, n_frames, src, "src", src_frame_stride, (int64_t)width * height * (g.depth16 ? 1 : 3), out,
                             out_capacity, out_offsets, out_sizes, g.n_strips, "strips");
    if (rc != SGS_OK) return rc;
    const int64_t n = (int64_t)n_frames * g.n_strips;
    PngScratch& Z = ctx->png;
    sgs::PngJob J;
    memset(&J, 0, sizeof J);
    if ((rc = ready_file_sink(ctx, Z.files, n, out, out_capacity, out_offsets, out_sizes, J.sink)) != SGS_OK || n == 0) return rc;
    const int64_t slot = (((int64_t)std::min(g.rows_per_strip, height) * (g.row_bytes + 1) + 16) + 15) & ~(int64_t)15;
    SGS_HIP(ctx, Z.rec.grow(n, Grow::geometric));
    SGS_HIP(ctx, Z.slots.grow(n * slot, Grow::geometric));
    SGS_HIP(ctx, Z.adler.grow(n_frames, Grow::geometric));
    J.src = src; J.frame_stride = src_frame_stride; J.width = width; J.height = height; J.depth16 = g.depth16;
    J.scale = params->depth_scale; J.dmax = params->depth_max; J.bpp = g.bpp; J.row_bytes = g.row_bytes;
    J.rows_per_strip = g.rows_per_strip; J.n_strips = g.n_strips; J.n_frames = n_frames;
    J.slot = slot; J.slots = Z.slots.p; J.rec = Z.rec.p; J.adler = Z.adler.p;
    sgs::png::build_head(J.head, width, height, g.depth16 != 0);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(sgs::k_png_strips, dim3((unsigned)n), dim3(64), 0, st, J);
    hipLaunchKernelGGL(sgs::k_png_scan, dim3(1), dim3(SGS_PNG_SCAN_THREADS), 0, st, J);
    hipLaunchKernelGGL(sgs::k_png_gather, dim3((unsigned)n), dim3(SGS_PNG_GATHER_THREADS), 0, st, J);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

int sgs_png_status(sgs_ctx* ctx, int64_t* bytes_needed) {
    return file_status(ctx, "sgs_encode_png", ctx ? &ctx->png.files : nullptr, bytes_needed);
}

}  // extern "C"

// ---- resize (csrc/sgs_resize.h) ---------------------------------------------------------------------------------------------------
namespace {

// The tap table of one axis on the device: the context's own of these sizes, built and uploaded on first use (a synchronous copy, so
// it is complete before any launch that follows).
int resize_axis(sgs_ctx* ctx, int in, int out, int filter, int format, sgs::ResizeAxis& A) {
    ResizeScratch& Z = ctx->resize;
    const ResizeScratch::Entry* hit = nullptr;
    for (const ResizeScratch::Entry& e : Z.tables)
        if (e.in == in && e.out == out && e.filter == filter && e.format == format) hit = &e;
    if (!hit) {
        const bool fixed = format == SGS_RESIZE_RGB8;
        sgs::resize::AxisTable T;
        sgs::resize::build_axis(in, out, fixed, T);
        ResizeScratch::Entry e = {in, out, filter, format, T.ksize, {}, {}};
        const void* w = fixed ? static_cast<const void*>(T.ki.data()) : static_cast<const void*>(T.kd.data());
        const size_t w_bytes = fixed ? T.ki.size() * sizeof(int) : T.kd.size() * sizeof(double);
        SGS_HIP(ctx, e.bounds.grow((int64_t)T.bounds.size()));
        SGS_HIP(ctx, e.weights.grow((int64_t)w_bytes));
        SGS_HIP(ctx, hipMemcpy(e.bounds.p, T.bounds.data(), T.bounds.size() * sizeof(int), hipMemcpyHostToDevice));
        SGS_HIP(ctx, hipMemcpy(e.weights.p, w, w_bytes, hipMemcpyHostToDevice));
        Z.tables.push_back(std::move(e));      // only a filled table is remembered; never trimmed: a few KB per pair of sizes a context has seen
        hit = &Z.tables.back();
    }
    A.bounds = hit->bounds.p; A.ksize = hit->ksize;
    A.ki = format == SGS_RESIZE_RGB8 ? reinterpret_cast<const int*>(hit->weights.p) : nullptr;
    A.kd = format == SGS_RESIZE_RGB8 ? nullptr : reinterpret_cast<const double*>(hit->weights.p);
    return SGS_OK;
}

template <int FMT>
void resize_launch(const sgs::ResizeJob& J, int filter, bool do_h, bool do_v, int n_frames, hipStream_t st) {
    const dim3 block(SGS_RESIZE_THREADS);
    auto grid = [&](long long pixels) { return dim3((unsigned)((pixels + SGS_RESIZE_THREADS - 1) / SGS_RESIZE_THREADS), (unsigned)n_frames); };
    if (filter == SGS_RESIZE_LINEAR) {
        hipLaunchKernelGGL(sgs::k_resize_linear<FMT>, grid((long long)J.w * J.h), block, 0, st, J);
        return;
    }
    if (!do_h && !do_v) hipLaunchKernelGGL(sgs::k_resize_copy<FMT>, grid((long long)J.w * J.h), block, 0, st, J);
    if (do_h) hipLaunchKernelGGL(sgs::k_resize_h<FMT>, grid((long long)J.w * J.H), block, 0, st, J);
    if (do_v) hipLaunchKernelGGL(sgs::k_resize_v<FMT>, grid((long long)J.w * J.h), block, 0, st, J);
}

}  // namespace

extern "C" {

void sgs_resize_params_default(sgs_resize_params* p) {
    if (!p) return;
    p->format = SGS_RESIZE_RGB8; p->filter = SGS_RESIZE_BICUBIC; p->dst_width = 320; p->dst_height = 240;
    p->clip_lo = -INFINITY; p->clip_hi = INFINITY; p->reserved[0] = p->reserved[1] = 0;
}

int sgs_resize(sgs_ctx* ctx, const float* src, int width, int height, int n_frames, int64_t src_frame_stride,
               const sgs_resize_params* p, float* dst, int64_t dst_frame_stride, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_resize"; const Args a = {ctx, who};
    if (!p) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: params is NULL", who);
    if (p->format != SGS_RESIZE_RGB8 && p->format != SGS_RESIZE_F32)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: format %d is neither SGS_RESIZE_RGB8 nor SGS_RESIZE_F32", who, p->format);
    if (p->filter != SGS_RESIZE_BICUBIC && p->filter != SGS_RESIZE_LINEAR)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: filter %d is neither SGS_RESIZE_BICUBIC nor SGS_RESIZE_LINEAR", who, p->filter);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = {%d, %d}, must be 0", who, p->reserved[0], p->reserved[1]);
    if (n_frames < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    if (width < 1 || height < 1 || width > 65535 || height > 65535) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: source %d x %d is outside 1..65535", who, width, height);
    if (p->dst_width < 1 || p->dst_height < 1 || p->dst_width > 65535 || p->dst_height > 65535)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: destination %d x %d is outside 1..65535", who, p->dst_width, p->dst_height);
    if (std::isnan(p->clip_lo) || std::isnan(p->clip_hi)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: clip bound is NaN", who);
    if (p->clip_lo > p->clip_hi) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: clip_lo %g is above clip_hi %g", who, (double)p->clip_lo, (double)p->clip_hi);
    if (n_frames == 0) return SGS_OK;          // nothing to do, whatever the pointers are: only the parameters are judged
    SGS_TRY(a.non_null(src, "src", dst, "dst"));
    const int ch = p->format == SGS_RESIZE_RGB8 ? 3 : 1;
    const int64_t src_floats = (int64_t)width * height * ch, dst_floats = (int64_t)p->dst_width * p->dst_height * ch;
    if (n_frames > 1) {                        // one frame has no stride to judge (sgs_object_table and sgs_topdown_map judge it all the same)
        SGS_TRY(a.frames_fit(src_frame_stride, src_floats, "src frames overlap (stride %lld floats, a frame has %lld)"));
        SGS_TRY(a.frames_fit(dst_frame_stride, dst_floats, "dst frames overlap (stride %lld floats, a frame has %lld)"));
    }
    if (Args::overlap(src, (uint64_t)(((int64_t)(n_frames - 1) * src_frame_stride + src_floats) * 4),
                      dst, (uint64_t)(((int64_t)(n_frames - 1) * dst_frame_stride + dst_floats) * 4)))
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: src and dst overlap", who);       // (without the pointers, unlike disjoint's)
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    sgs::ResizeJob J;
    memset(&J, 0, sizeof J);
    J.W = width; J.H = height; J.w = p->dst_width; J.h = p->dst_height;
    J.src_stride = src_frame_stride; J.dst_stride = dst_frame_stride; J.clip_lo = p->clip_lo; J.clip_hi = p->clip_hi;
    const bool bicubic = p->filter == SGS_RESIZE_BICUBIC;
    const bool do_h = bicubic && J.W != J.w, do_v = bicubic && J.H != J.h;
    J.h_to_dst = !do_v; J.v_from_src = !do_h;
    int rc;
    if (do_h && (rc = resize_axis(ctx, J.W, J.w, p->filter, p->format, J.ax)) != SGS_OK) return rc;
    if (do_v && (rc = resize_axis(ctx, J.H, J.h, p->filter, p->format, J.ay)) != SGS_OK) return rc;
    const int kMaxFrames = 65535;              // gridDim.y
    if (do_h && do_v) SGS_HIP(ctx, ctx->resize.mid.grow((int64_t)std::min(n_frames, kMaxFrames) * J.H * J.w, Grow::geometric));
    J.mid = ctx->resize.mid.p;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    for_chunks(n_frames, kMaxFrames, [&](int f0, int n) {
        J.src = src + (int64_t)f0 * src_frame_stride; J.dst = dst + (int64_t)f0 * dst_frame_stride;
        if (p->format == SGS_RESIZE_RGB8) resize_launch<sgs::RESIZE_RGB8>(J, p->filter, do_h, do_v, n, st);
        else resize_launch<sgs::RESIZE_F32>(J, p->filter, do_h, do_v, n, st);
    });
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_object_table ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(sgs_object_row) == sizeof(sgs::ObjRow) && alignof(sgs_object_row) == 8, "sgs_object_row is 40 bytes, 8-byte aligned");

extern "C" {

int sgs_object_table(sgs_ctx* ctx, const int32_t* ids, const float* depth, int n_frames, int height, int width, int64_t frame_stride,
                     int32_t n_labels, sgs_object_row* out_rows, uint32_t* out_counts, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_object_table"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(ids, "ids", out_rows, "out_rows", out_counts, "out_counts"));          // depth may be null (no depth channel); if given it is aligned, below
    if (n_frames < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    if (height < 1 || width < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: frame %d x %d", who, width, height);
    const int64_t pixels = (int64_t)height * width;
    if (pixels > 0x7FFFFFFFll) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: frame %d x %d has more than 2^31 - 1 pixels", who, width, height);
    SGS_TRY(a.frames_fit(frame_stride, pixels, "frames overlap (stride %lld elements, a frame has %lld)"));      // for one frame too
    if (n_labels < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_labels = %d", who, (int)n_labels);
    // the kernels' atomics are 64-bit on sum_x / sum_y and 32-bit elsewhere; a misaligned one must never reach the device
    if (reinterpret_cast<uintptr_t>(out_rows) % 8) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: out_rows %p is not 8-byte aligned", who, (const void*)out_rows);
    if (reinterpret_cast<uintptr_t>(ids) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: ids %p is not 4-byte aligned", who, (const void*)ids);
    if (reinterpret_cast<uintptr_t>(depth) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: depth %p is not 4-byte aligned", who, (const void*)depth);
    if (reinterpret_cast<uintptr_t>(out_counts) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: out_counts %p is not 4-byte aligned", who, (const void*)out_counts);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::ObjJob J;
    J.ids = ids; J.depth = depth; J.rows = reinterpret_cast<sgs::ObjRow*>(out_rows); J.counts = out_counts;
    J.stride = frame_stride; J.W = width; J.H = height; J.n_labels = n_labels; J.n_frames = n_frames;
    const int64_t n_rows = (int64_t)n_frames * n_labels;
    const int64_t clear_blocks = std::min<int64_t>((std::max<int64_t>(n_rows, 2ll * n_frames) + SGS_OBJ_THREADS - 1) / SGS_OBJ_THREADS, 65536);
    hipLaunchKernelGGL(sgs::k_obj_clear, dim3((unsigned)clear_blocks), dim3(SGS_OBJ_THREADS), 0, st, J);
    const unsigned regions = (unsigned)((pixels + SGS_OBJ_REGION - 1) / SGS_OBJ_REGION);
    for_chunks(n_frames, SGS_OBJ_MAX_FRAMES, [&](int f0, int n) {
        sgs::ObjJob K = J;
        K.ids = ids + (int64_t)f0 * frame_stride; K.depth = depth ? depth + (int64_t)f0 * frame_stride : nullptr;
        K.rows = J.rows + (int64_t)f0 * n_labels; K.counts = out_counts + 2ll * f0; K.n_frames = n;
        hipLaunchKernelGGL(sgs::k_obj_reduce, dim3(regions, (unsigned)n), dim3(SGS_OBJ_THREADS), 0, st, K);
    });
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_image_similarity (csrc/sgs_similarity.h) --------------------------------------------------------------------------------------
static_assert(sizeof(sgs_similarity_row) == sizeof(sgs::SimRow) && alignof(sgs_similarity_row) == 8, "sgs_similarity_row is 64 bytes, 8-byte aligned");

extern "C" {

int sgs_image_similarity(sgs_ctx* ctx, const float* rgb, int width, int height, int n_frames, int64_t rgb_frame_stride,
                         const uint8_t* target, int64_t target_frame_stride, sgs_similarity_row* out_rows, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_image_similarity"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(rgb, "rgb", target, "target", out_rows, "out_rows"));
    if (n_frames < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    if (width < SGS_SIM_WINDOW || width > 65535) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: width %d is outside %d..65535 (a window is %d pixels wide)", who, width, SGS_SIM_WINDOW, SGS_SIM_WINDOW);
    if (height < SGS_SIM_WINDOW || height > 65535) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: height %d is outside %d..65535 (a window is %d pixels high)", who, height, SGS_SIM_WINDOW, SGS_SIM_WINDOW);
    const int64_t frame = 3ll * width * height;
    SGS_TRY(a.frames_fit(rgb_frame_stride, frame, "rgb_frame_stride %lld floats is smaller than a frame (%lld)"));       // for one frame too
    if (target_frame_stride != 0 && target_frame_stride < frame)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: target_frame_stride %lld bytes is neither 0 nor a frame (%lld) or more", who, (long long)target_frame_stride, (long long)frame);
    // the rows are updated with 64-bit atomics; a misaligned one must never reach the device
    SGS_TRY(a.aligned(8, out_rows, "out_rows"));
    SGS_TRY(a.aligned(4, rgb, "rgb"));
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::SimJob J;
    J.rgb = rgb; J.target = target; J.rows = reinterpret_cast<sgs::SimRow*>(out_rows);
    J.rgb_stride = rgb_frame_stride; J.target_stride = target_frame_stride; J.W = width; J.H = height; J.n_frames = n_frames;
    const int nwx = width - (SGS_SIM_WINDOW - 1), nwy = height - (SGS_SIM_WINDOW - 1);
    const int tiles_x = (nwx + SGS_SIM_TILE_W - 1) / SGS_SIM_TILE_W;
    const int tiles_y = (nwy + SGS_SIM_TILE_H - 1) / SGS_SIM_TILE_H;
    J.tiles_x = tiles_x;
    const unsigned clear_blocks = (unsigned)std::min<int64_t>(((int64_t)n_frames + SGS_SIM_THREADS - 1) / SGS_SIM_THREADS, 65536);
    hipLaunchKernelGGL(sgs::k_sim_clear, dim3(clear_blocks), dim3(SGS_SIM_THREADS), 0, st, J);
    for_chunks(n_frames, SGS_SIM_MAX_FRAMES, [&](int f0, int n) {
        sgs::SimJob K = J;
        K.rgb = rgb + (int64_t)f0 * rgb_frame_stride; K.target = target + (int64_t)f0 * target_frame_stride; K.rows = J.rows + f0; K.n_frames = n;
        hipLaunchKernelGGL(sgs::k_sim_reduce, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(SGS_SIM_THREADS), 0, st, K);
    });
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_topdown_map, sgs_topdown_summary (csrc/sgs_topdown.h) -------------------------------------------------------------------------
static_assert(sizeof(sgs_topdown_params) == 52, "sgs_topdown_params is thirteen 4-byte fields");

extern "C" {

void sgs_topdown_params_default(sgs_topdown_params* p) {
    if (!p) return;
    p->nx = 256; p->ny = 256; p->origin_x = -6.4f; p->origin_y = -6.4f; p->cell_size = 0.05f;
    p->min_z = 0.1f; p->max_z = 6.5f; p->free_lo = -0.15f; p->free_hi = 0.15f; p->occ_lo = 0.15f; p->occ_hi = 1.5f;
    p->flags = SGS_TOPDOWN_CLEAR; p->reserved = 0;
}

int sgs_topdown_map(sgs_ctx* ctx, const float* depth, int width, int height, int n_frames, int64_t frame_stride,
                    const float* pix_to_map, const sgs_topdown_params* p, uint32_t* grid, uint32_t* out_counts, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_topdown_map"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(depth, "depth", pix_to_map, "pix_to_map", p, "params", grid, "grid", out_counts, "out_counts"));
    if (n_frames < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames = %d", who, n_frames);
    if (height < 1 || width < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: frame %d x %d", who, width, height);
    const int64_t pixels = (int64_t)height * width;
    if (pixels > 0x7FFFFFFFll) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: frame %d x %d has more than 2^31 - 1 pixels", who, width, height);
    SGS_TRY(a.frames_fit(frame_stride, pixels, "frames overlap (frame_stride %lld elements, a frame has %lld)"));        // for one frame too
    if ((int64_t)n_frames * pixels > 0xFFFFFFFFll)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_frames * height * width = %lld could pass 2^32 - 1 hits in one cell", who, (long long)((int64_t)n_frames * pixels));
    if (p->nx < 1 || p->ny < 1 || 2ll * p->nx * p->ny > 0x7FFFFFFFll)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: nx = %d, ny = %d (1 <= nx, ny and 2 nx ny <= 2^31 - 1)", who, (int)p->nx, (int)p->ny);
    if (!std::isfinite(p->cell_size) || p->cell_size <= 0.0f) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: cell_size = %g (finite and > 0)", who, (double)p->cell_size);
    if (!std::isfinite(p->origin_x) || !std::isfinite(p->origin_y))
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: origin (%g, %g) is not finite", who, (double)p->origin_x, (double)p->origin_y);
    if (!(p->min_z <= p->max_z)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: min_z %g is not <= max_z %g", who, (double)p->min_z, (double)p->max_z);
    if (!std::isfinite(p->free_lo) || !std::isfinite(p->free_hi) || p->free_lo > p->free_hi)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: free band [%g, %g] (finite, free_lo <= free_hi)", who, (double)p->free_lo, (double)p->free_hi);
    if (!std::isfinite(p->occ_lo) || !std::isfinite(p->occ_hi) || p->occ_lo > p->occ_hi)
        SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: occupied band (%g, %g] (finite, occ_lo <= occ_hi)", who, (double)p->occ_lo, (double)p->occ_hi);
    if (p->flags & ~SGS_TOPDOWN_CLEAR) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %d", who, (int)p->reserved);
    // the kernels' atomics are 32-bit; a misaligned one must never reach the device
    const struct { const void* at; const char* name; } buffers[] = {{depth, "depth"}, {pix_to_map, "pix_to_map"}, {grid, "grid"}, {out_counts, "out_counts"}};
    for (const auto& b : buffers)
        if (reinterpret_cast<uintptr_t>(b.at) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %s %p is not 4-byte aligned", who, b.name, b.at);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::TopdownJob J;
    J.depth = depth; J.P = pix_to_map; J.grid = grid; J.counts = out_counts;
    J.stride = frame_stride; J.W = width; J.H = height; J.n_frames = n_frames; J.nx = p->nx; J.ny = p->ny;
    J.origin_x = p->origin_x; J.origin_y = p->origin_y; J.inv = 1.0f / p->cell_size;
    J.min_z = p->min_z; J.max_z = p->max_z; J.free_lo = p->free_lo; J.free_hi = p->free_hi; J.occ_lo = p->occ_lo; J.occ_hi = p->occ_hi;
    J.clear = p->flags & SGS_TOPDOWN_CLEAR;
    const int64_t clear_words = std::max<int64_t>(4ll * n_frames, J.clear ? 2ll * p->nx * p->ny : 0);
    const int64_t clear_blocks = std::min<int64_t>((clear_words + SGS_TOPDOWN_THREADS - 1) / SGS_TOPDOWN_THREADS, 65536);
    hipLaunchKernelGGL(sgs::k_topdown_clear, dim3((unsigned)clear_blocks), dim3(SGS_TOPDOWN_THREADS), 0, st, J);
    const unsigned regions = (unsigned)((pixels + SGS_TOPDOWN_REGION - 1) / SGS_TOPDOWN_REGION);
    for_chunks(n_frames, SGS_TOPDOWN_MAX_FRAMES, [&](int f0, int n) {
        sgs::TopdownJob K = J;
        K.depth = depth + (int64_t)f0 * frame_stride; K.P = pix_to_map + 12ll * f0; K.counts = out_counts + 4ll * f0; K.n_frames = n;
        hipLaunchKernelGGL(sgs::k_topdown_map, dim3(regions, (unsigned)n), dim3(SGS_TOPDOWN_THREADS), 0, st, K);
    });
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

int sgs_topdown_summary(sgs_ctx* ctx, const uint32_t* grid, int nx, int ny, uint32_t min_hits, uint64_t* out, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_topdown_summary"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(grid, "grid", out, "out"));
    if (nx < 1 || ny < 1 || 2ll * nx * ny > 0x7FFFFFFFll) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: nx = %d, ny = %d (1 <= nx, ny and 2 nx ny <= 2^31 - 1)", who, nx, ny);
    if (min_hits < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: min_hits = 0", who);
    if (reinterpret_cast<uintptr_t>(grid) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: grid %p is not 4-byte aligned", who, (const void*)grid);
    // out is updated with 64-bit atomics; a misaligned one must never reach the device
    if (reinterpret_cast<uintptr_t>(out) % 8) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: out %p is not 8-byte aligned", who, (const void*)out);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const long long cells = (long long)nx * ny;
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    hipLaunchKernelGGL(sgs::k_topdown_sum_clear, dim3(1), dim3(64), 0, st, o);
    const unsigned blocks = (unsigned)std::min<long long>((cells + SGS_TOPDOWN_THREADS - 1) / SGS_TOPDOWN_THREADS, SGS_TOPDOWN_SUM_BLOCKS);
    hipLaunchKernelGGL(sgs::k_topdown_sum, dim3(blocks), dim3(SGS_TOPDOWN_THREADS), 0, st, grid, cells, (unsigned)min_hits, o);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_clearance_map, sgs_clearance_query (csrc/sgs_clearance.h) ----------------------------------------------------------------------
static_assert(sizeof(sgs_clearance_params) == 28, "sgs_clearance_params is seven 4-byte fields");
static_assert(sizeof(sgs_clearance_frame) == 64, "sgs_clearance_frame is five doubles, four 4-byte fields and an int64");
static_assert(SGS_CLEARANCE_NONE == SGS_CLEAR_NONE && SGS_CLEARANCE_SRC_MASK8 == SGS_CLEAR_SRC_MASK8 && SGS_CLEARANCE_SRC_TOPDOWN == SGS_CLEAR_SRC_TOPDOWN &&
              SGS_CLEARANCE_UNSEEN_BLOCKS == SGS_CLEAR_UNSEEN_BLOCKS && SGS_CLEARANCE_NEGATE == SGS_CLEAR_NEGATE && SGS_CLEARANCE_FLIP_X == SGS_CLEAR_FLIP_X &&
              SGS_CLEARANCE_FLIP_Y == SGS_CLEAR_FLIP_Y, "the kernels' constants are the header's");

extern "C" {

int sgs_clearance_map(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_clearance_params* p,
                      uint32_t* work, uint32_t* d2, uint32_t* out_counts, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_clearance_map"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(src, "src", p, "params", work, "work", d2, "d2", out_counts, "out_counts"));
    if (n_maps < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_maps = %d", who, n_maps);
    SGS_TRY(a.grid_within(p->nx, p->ny, SGS_CLEAR_MAX_NX));
    if (p->source != SGS_CLEARANCE_SRC_MASK8 && p->source != SGS_CLEARANCE_SRC_TOPDOWN) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown source %d", who, (int)p->source);
    const bool topdown = p->source == SGS_CLEARANCE_SRC_TOPDOWN;
    const int64_t cells = (int64_t)p->nx * p->ny, map_elements = topdown ? 2 * cells : cells;
    SGS_TRY(a.frames_fit(map_stride, map_elements, "maps overlap (map_stride %lld elements, a map has %lld)"));          // for one map too
    if ((p->flags & ~SGS_CLEARANCE_UNSEEN_BLOCKS) || (p->flags && !topdown)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x for source %d", who, (unsigned)p->flags, (int)p->source);
    if (topdown && p->min_hits < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: min_hits = 0", who);
    if (p->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %d", who, (int)p->reserved);
    const uint64_t out_bytes = 4ull * (uint64_t)n_maps * (uint64_t)cells;
    SGS_TRY(a.disjoint(d2, out_bytes, "d2", work, out_bytes, "work"));
    // the kernels' loads, stores and atomics are 32-bit; a misaligned one must never reach the device (src: a seen map only, a mask is bytes)
    const struct { const void* at; const char* name; bool words; } buffers[] = {{src, "src", topdown}, {work, "work", true}, {d2, "d2", true}, {out_counts, "out_counts", true}};
    for (const auto& b : buffers)
        if (b.words && reinterpret_cast<uintptr_t>(b.at) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: %s %p is not 4-byte aligned", who, b.name, b.at);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::ClearanceJob J;
    J.src = src; J.work = work; J.d2 = d2; J.counts = out_counts; J.stride = map_stride; J.map0 = 0;
    J.nx = p->nx; J.ny = p->ny; J.n_maps = n_maps; J.kind = p->source;
    J.min_hits = p->min_hits; J.unseen_blocks = p->flags & SGS_CLEARANCE_UNSEEN_BLOCKS; J.max_d2 = p->max_d2;
    const int64_t count_words = 4ll * n_maps;
    const unsigned clear_blocks = (unsigned)std::min<int64_t>((count_words + SGS_CLEAR_THREADS - 1) / SGS_CLEAR_THREADS, 1024);
    hipLaunchKernelGGL(sgs::k_clear_counts, dim3(clear_blocks), dim3(SGS_CLEAR_THREADS), 0, st, out_counts, (long long)count_words);
    const unsigned row_groups = (unsigned)((p->ny + SGS_CLEAR_ROWS - 1) / SGS_CLEAR_ROWS), words = (unsigned)((p->nx + 63) / 64);
    for_chunks(n_maps, SGS_CLEAR_MAX_MAPS, [&](int m0, int n) {
        sgs::ClearanceJob K = J;
        K.map0 = m0; K.n_maps = n;
        hipLaunchKernelGGL(sgs::k_clear_rows, dim3(row_groups, (unsigned)n), dim3(SGS_CLEAR_THREADS), 0, st, K);
        hipLaunchKernelGGL(sgs::k_clear_cols, dim3(words, row_groups, (unsigned)n), dim3(SGS_CLEAR_THREADS), 0, st, K);
    });
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

int sgs_clearance_query(sgs_ctx* ctx, const uint32_t* d2, int nx, int ny, const double* segs, int n,
                        const sgs_clearance_frame* f, uint32_t* out, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_clearance_query"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(d2, "d2", segs, "segs", f, "frame", out, "out"));
    if (n < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n = %d", who, n);
    SGS_TRY(a.grid_within(nx, ny, SGS_CLEAR_MAX_NX));
    if (!std::isfinite(f->scale) || f->scale <= 0.0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: scale = %g (finite and > 0)", who, f->scale);
    if (!std::isfinite(f->min_x) || !std::isfinite(f->min_y)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: min (%g, %g) is not finite", who, f->min_x, f->min_y);
    if (!std::isfinite(f->sum_x) || !std::isfinite(f->sum_y)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: sum (%g, %g) is not finite", who, f->sum_x, f->sum_y);
    if (f->margin < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: margin = %d", who, (int)f->margin);
    if (f->flags & ~(SGS_CLEARANCE_NEGATE | SGS_CLEARANCE_FLIP_X | SGS_CLEARANCE_FLIP_Y)) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)f->flags);
    if (f->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %lld", who, (long long)f->reserved);
    if (reinterpret_cast<uintptr_t>(d2) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: d2 %p is not 4-byte aligned", who, (const void*)d2);
    if (reinterpret_cast<uintptr_t>(out) % 4) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: out %p is not 4-byte aligned", who, (const void*)out);
    if (reinterpret_cast<uintptr_t>(segs) % 8) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: segs %p is not 8-byte aligned", who, (const void*)segs);
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::ClearanceQuery Q;
    Q.d2 = d2; Q.segs = segs; Q.out = out; Q.n = n; Q.nx = nx; Q.ny = ny; Q.margin = f->margin; Q.n_samples = f->n_samples;
    Q.min_x = f->min_x; Q.min_y = f->min_y; Q.sum_x = f->sum_x; Q.sum_y = f->sum_y; Q.scale = f->scale; Q.flags = f->flags; Q.max_d2 = f->max_d2;
    hipLaunchKernelGGL(sgs::k_clear_query, dim3((unsigned)((n + SGS_CLEAR_THREADS - 1) / SGS_CLEAR_THREADS)), dim3(SGS_CLEAR_THREADS), 0, st, Q);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_geodesic_field, sgs_geodesic_path (csrc/sgs_geodesic.h) --------------------------------------------------------------------------
static_assert(sizeof(sgs_geodesic_params) == 24, "sgs_geodesic_params is six 4-byte fields");
static_assert(SGS_GEODESIC_NONE == SGS_GEO_NONE && SGS_GEODESIC_SRC_MASK8 == SGS_GEO_SRC_MASK8 && SGS_GEODESIC_SRC_D2 == SGS_GEO_SRC_D2 &&
              SGS_GEODESIC_MAX_N == SGS_GEO_MAX_N && SGS_GEODESIC_MAX_FIELDS == SGS_GEO_MAX_FIELDS && SGS_GEODESIC_PATH_MAX_FIELDS == SGS_GEO_PATH_MAX_FIELDS,
              "the kernels' constants are the header's");

// What sgs_geodesic_field and sgs_geodesic_path refuse alike: the map, the params and the field table (a HOST array).
static int geodesic_check(const Args& a, const void* src, int n_maps, int64_t map_stride, const sgs_geodesic_params* p,
                          const int32_t* field_map, int n_fields, int max_fields) {
    sgs_ctx* ctx = a.ctx; const char* who = a.who;
    SGS_TRY(a.non_null(src, "src", p, "params", field_map, "field_map"));
    if (n_maps < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_maps = %d", who, n_maps);
    if (n_fields < 1 || n_fields > max_fields) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_fields = %d (1 <= n_fields <= %d)", who, n_fields, max_fields);
    SGS_TRY(a.grid_within(p->nx, p->ny, SGS_GEO_MAX_N));
    if (p->source != SGS_GEODESIC_SRC_MASK8 && p->source != SGS_GEODESIC_SRC_D2) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown source %d", who, (int)p->source);
    if (p->flags & ~SGS_GEODESIC_CONTINUE) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %d", who, (int)p->reserved);
    SGS_TRY(a.frames_fit(map_stride, (int64_t)p->nx * p->ny, "maps overlap (map_stride %lld elements, a map has %lld)"));
    for (int f = 0; f < n_fields; ++f)         // field_map is a HOST array, read here: nothing has been enqueued yet
        if (field_map[f] < 0 || field_map[f] >= n_maps) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: field_map[%d] = %d (n_maps = %d)", who, f, (int)field_map[f], n_maps);
    return p->source == SGS_GEODESIC_SRC_D2 ? a.aligned(4, src, "src") : SGS_OK;              // a mask is read byte by byte
}

extern "C" {

int sgs_geodesic_tile(void) { return SGS_GEO_TILE; }

int64_t sgs_geodesic_state_words(int nx, int ny, int n_fields) {
    if (nx < 1 || ny < 1 || nx > SGS_GEO_MAX_N || ny > SGS_GEO_MAX_N || n_fields < 1 || n_fields > SGS_GEO_MAX_FIELDS) return -1;
    const int64_t tiles = (int64_t)((nx + SGS_GEO_TILE - 1) / SGS_GEO_TILE) * ((ny + SGS_GEO_TILE - 1) / SGS_GEO_TILE);
    return (int64_t)n_fields * (2 + tiles);
}

int sgs_geodesic_field(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_geodesic_params* p,
                       const int32_t* field_map, int n_fields, const int32_t* seeds, int n_seeds,
                       uint32_t* dist, uint32_t* state, int rounds, uint32_t* status, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_geodesic_field"; const Args a = {ctx, who};
    SGS_TRY(geodesic_check(a, src, n_maps, map_stride, p, field_map, n_fields, SGS_GEO_MAX_FIELDS));
    SGS_TRY(a.non_null(seeds, "seeds", dist, "dist", state, "state", status, "status"));
    if (n_seeds < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_seeds = %d", who, n_seeds);
    if (rounds < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: rounds = %d", who, rounds);
    for (int s = 0; s < n_seeds; ++s) {        // seeds is a HOST array, as field_map is
        const int32_t* e = seeds + 3 * (size_t)s;
        if (e[0] < 0 || e[0] >= n_fields) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: seeds[%d] names field %d (n_fields = %d)", who, s, (int)e[0], n_fields);
        if (e[1] < 0 || e[1] >= p->nx || e[2] < 0 || e[2] >= p->ny)
            SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: seeds[%d] = (%d, %d) is outside the grid %d x %d", who, s, (int)e[1], (int)e[2], (int)p->nx, (int)p->ny);
    }
    SGS_TRY(a.aligned(8, dist, "dist"));
    SGS_TRY(a.aligned(4, state, "state", status, "status"));
    const int64_t cells = (int64_t)p->nx * p->ny, state_words = sgs_geodesic_state_words(p->nx, p->ny, n_fields);
    SGS_TRY(a.disjoint(dist, 8ull * (uint64_t)n_fields * (uint64_t)cells, "dist", state, 4ull * (uint64_t)state_words, "state"));
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::GeodesicJob J;
    J.src = src; J.dist = reinterpret_cast<unsigned long long*>(dist); J.state = state; J.stride = map_stride;
    J.nx = p->nx; J.ny = p->ny; J.n_fields = n_fields; J.kind = p->source; J.max_d2 = p->max_d2;
    J.tiles_x = (p->nx + SGS_GEO_TILE - 1) / SGS_GEO_TILE; J.tiles_y = (p->ny + SGS_GEO_TILE - 1) / SGS_GEO_TILE;
    J.colour_x = J.colour_y = 0;
    if (!(p->flags & SGS_GEODESIC_CONTINUE)) {
        const int64_t pairs = (int64_t)n_fields * cells, zero_words = state_words - n_fields;
        const unsigned blocks = (unsigned)std::min<int64_t>((std::max(pairs, zero_words) + SGS_GEO_THREADS - 1) / SGS_GEO_THREADS, 4096);
        hipLaunchKernelGGL(sgs::k_geo_fill, dim3(blocks), dim3(SGS_GEO_THREADS), 0, st, J.dist, (long long)pairs, state + n_fields, (long long)zero_words);
        for_chunks(n_fields, SGS_GEO_PUT_WORDS, [&](int f0, int n) {                 // the field table travels in kernel arguments: no host buffer outlives the call
            sgs::GeodesicWords W;
            for (int k = 0; k < SGS_GEO_PUT_WORDS; ++k) W.w[k] = k < n ? (unsigned)field_map[f0 + k] : 0u;
            hipLaunchKernelGGL(sgs::k_geo_put, dim3(1), dim3(SGS_GEO_PUT_WORDS), 0, st, state + f0, W, n);
        });
        for_chunks(n_seeds, SGS_GEO_SEEDS_PER_LAUNCH, [&](int s0, int n) {
            sgs::GeodesicSeeds S;
            for (int k = 0; k < SGS_GEO_SEEDS_PER_LAUNCH; ++k)
                for (int c = 0; c < 3; ++c) S.s[k][c] = k < n ? seeds[3 * (size_t)(s0 + k) + c] : 0;
            hipLaunchKernelGGL(sgs::k_geo_seed, dim3(1), dim3(SGS_GEO_SEEDS_PER_LAUNCH), 0, st, J, S, n);
        });
    }
    for (int r = 0; r < rounds; ++r)
        for (int colour = 0; colour < 4; ++colour) {
            sgs::GeodesicJob K = J;
            K.colour_x = colour & 1; K.colour_y = colour >> 1;
            const int cx = (J.tiles_x - K.colour_x + 1) / 2, cy = (J.tiles_y - K.colour_y + 1) / 2;      // the tiles of this colour
            if (cx < 1 || cy < 1) continue;
            hipLaunchKernelGGL(sgs::k_geo_relax, dim3((unsigned)cx, (unsigned)cy, (unsigned)n_fields), dim3(SGS_GEO_THREADS), 0, st, K);
        }
    hipLaunchKernelGGL(sgs::k_geo_status, dim3((unsigned)n_fields), dim3(SGS_GEO_THREADS), 0, st, J, status);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

int sgs_geodesic_path(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_geodesic_params* p,
                      const int32_t* field_map, int n_fields, const uint32_t* dist, const int32_t* queries, int n_queries,
                      int max_len, int32_t* out_cells, uint32_t* out_info, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_geodesic_path"; const Args a = {ctx, who};
    SGS_TRY(geodesic_check(a, src, n_maps, map_stride, p, field_map, n_fields, SGS_GEO_PATH_MAX_FIELDS));
    if (p->flags) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    SGS_TRY(a.non_null(dist, "dist", queries, "queries", out_cells, "out_cells", out_info, "out_info"));
    if (n_queries < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_queries = %d", who, n_queries);
    if (max_len < 1) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: max_len = %d", who, max_len);
    SGS_TRY(a.aligned(8, dist, "dist"));
    SGS_TRY(a.aligned(4, queries, "queries", out_cells, "out_cells", out_info, "out_info"));
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::GeodesicPathJob Q;
    Q.src = src; Q.dist = reinterpret_cast<const unsigned long long*>(dist); Q.queries = queries; Q.cells = out_cells; Q.info = out_info;
    Q.stride = map_stride; Q.nx = p->nx; Q.ny = p->ny; Q.n_fields = n_fields; Q.kind = p->source; Q.n = n_queries; Q.max_len = max_len; Q.max_d2 = p->max_d2;
    for (int f = 0; f < SGS_GEO_PATH_MAX_FIELDS; ++f) Q.field_map[f] = f < n_fields ? field_map[f] : 0;
    hipLaunchKernelGGL(sgs::k_geo_path, dim3((unsigned)((n_queries + SGS_GEO_THREADS - 1) / SGS_GEO_THREADS)), dim3(SGS_GEO_THREADS), 0, st, Q);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_regions_label (csrc/sgs_regions.h) ------------------------------------------------------------------------------------------------
static_assert(sizeof(sgs_regions_params) == 32, "sgs_regions_params is eight 4-byte fields");
static_assert(sizeof(sgs_region_row) == sizeof(sgs::RegRow) && alignof(sgs_region_row) == 8, "sgs_region_row is the kernels' RegRow");
static_assert(SGS_REGIONS_SRC_MASK8 == SGS_REG_SRC_MASK8 && SGS_REGIONS_SRC_D2 == SGS_REG_SRC_D2 && SGS_REGIONS_MAX_N == SGS_REG_MAX_N &&
              SGS_REGIONS_MAX_MAPS == SGS_REG_MAX_MAPS, "the kernels' constants are the header's");

extern "C" {

int sgs_regions_tile(void) { return SGS_REG_TILE; }

int64_t sgs_regions_work_words(int nx, int ny, int n_maps) {
    if (nx < 1 || ny < 1 || nx > SGS_REG_MAX_N || ny > SGS_REG_MAX_N || n_maps < 1 || n_maps > SGS_REG_MAX_MAPS) return -1;
    const int64_t cells = (int64_t)nx * ny, chunks = (cells + SGS_REG_CHUNK - 1) / SGS_REG_CHUNK;
    return (int64_t)n_maps * 2 * (cells + chunks);                                   // parent, root, two words per chunk
}

int sgs_regions_label(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_regions_params* p,
                      uint32_t* work, int32_t* labels, sgs_region_row* out_rows, int32_t max_regions,
                      uint32_t* out_counts, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_regions_label"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(src, "src", p, "params", work, "work", labels, "labels", out_counts, "out_counts"));
    if (max_regions < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: max_regions = %d", who, (int)max_regions);
    if (max_regions > 0) SGS_TRY(a.non_null(out_rows, "out_rows"));
    if (n_maps < 1 || n_maps > SGS_REG_MAX_MAPS) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_maps = %d (1 <= n_maps <= %d)", who, n_maps, SGS_REG_MAX_MAPS);
    SGS_TRY(a.grid_within(p->nx, p->ny, SGS_REG_MAX_N));
    if (p->source != SGS_REGIONS_SRC_MASK8 && p->source != SGS_REGIONS_SRC_D2) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown source %d", who, (int)p->source);
    if (p->connectivity != 4 && p->connectivity != 8) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown connectivity %d (4 or 8)", who, (int)p->connectivity);
    if (p->lo > p->hi) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: lo = %u > hi = %u", who, (unsigned)p->lo, (unsigned)p->hi);
    if (p->source == SGS_REGIONS_SRC_MASK8 && p->hi > 255u) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: hi = %u with a mask (hi <= 255)", who, (unsigned)p->hi);
    if (p->flags != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %d", who, (int)p->reserved);
    const int64_t cells = (int64_t)p->nx * p->ny;
    SGS_TRY(a.frames_fit(map_stride, cells, "maps overlap (map_stride %lld elements, a map has %lld)"));
    SGS_TRY(a.aligned(4, work, "work", labels, "labels", out_counts, "out_counts"));
    if (p->source == SGS_REGIONS_SRC_D2) SGS_TRY(a.aligned(4, src, "src"));          // a mask is read byte by byte
    SGS_TRY(a.aligned(8, out_rows, "out_rows"));
    const int64_t work_words = sgs_regions_work_words(p->nx, p->ny, n_maps);
    SGS_TRY(a.disjoint(labels, 4ull * (uint64_t)n_maps * (uint64_t)cells, "labels", work, 4ull * (uint64_t)work_words, "work"));
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    sgs::RegionsJob J;
    J.src = src; J.stride = map_stride; J.nx = p->nx; J.ny = p->ny; J.n_maps = n_maps; J.kind = p->source; J.conn = p->connectivity;
    J.lo = p->lo; J.hi = p->hi; J.cells = (unsigned)cells; J.max_regions = max_regions;
    J.tiles_x = (p->nx + SGS_REG_TILE - 1) / SGS_REG_TILE; J.tiles_y = (p->ny + SGS_REG_TILE - 1) / SGS_REG_TILE;
    J.n_chunks = (int)((cells + SGS_REG_CHUNK - 1) / SGS_REG_CHUNK);
    J.parent = work; J.root = work + (int64_t)n_maps * cells; J.chunks = work + 2 * (int64_t)n_maps * cells;
    J.labels = labels; J.rows = reinterpret_cast<sgs::RegRow*>(out_rows); J.counts = out_counts;
    const dim3 threads(SGS_REG_THREADS);
    const unsigned maps = (unsigned)n_maps, chunks = (unsigned)J.n_chunks;
    if (max_regions > 0) {
        const int64_t n_rows = (int64_t)n_maps * max_regions;
        hipLaunchKernelGGL(sgs::k_reg_clear, dim3((unsigned)std::min<int64_t>((n_rows + SGS_REG_THREADS - 1) / SGS_REG_THREADS, 4096)), threads, 0, st, J.rows, (long long)n_rows);
    }
    hipLaunchKernelGGL(sgs::k_reg_local, dim3((unsigned)J.tiles_x, (unsigned)J.tiles_y, maps), threads, 0, st, J);
    const int64_t border_cells = (int64_t)(J.tiles_y - 1) * p->nx + (int64_t)(J.tiles_x - 1) * p->ny;
    if (border_cells > 0)
        hipLaunchKernelGGL(sgs::k_reg_merge, dim3((unsigned)((border_cells + SGS_REG_THREADS - 1) / SGS_REG_THREADS), maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_flatten, dim3(chunks, maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_scan, dim3(maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_rank, dim3(chunks, maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_labels, dim3(chunks, maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_rows, dim3((unsigned)((cells + SGS_REG_ROW_REGION - 1) / SGS_REG_ROW_REGION), maps), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_reg_largest, dim3(maps), threads, 0, st, J);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"

// ---- sgs_endpoints (csrc/sgs_endpoints.h) ----------------------------------------------------------------------------------------------------
static_assert(sizeof(sgs_endpoints_params) == 28, "sgs_endpoints_params is seven 4-byte fields");
static_assert(sizeof(sgs_endpoints_item) == sizeof(sgs::EpItem) && alignof(sgs_endpoints_item) == 8, "sgs_endpoints_item is the kernels' EpItem");
static_assert(sizeof(sgs_endpoints_query) == sizeof(sgs::EpQuery) && sizeof(sgs_endpoints_answer) == sizeof(sgs::EpAnswer), "the kernels' query and answer are the header's");
static_assert(SGS_ENDPOINTS_SRC_MASK8 == SGS_EP_SRC_MASK8 && SGS_ENDPOINTS_SRC_D2 == SGS_EP_SRC_D2 && SGS_ENDPOINTS_MAX_N == SGS_EP_MAX_N &&
              SGS_ENDPOINTS_MAX_ITEMS == SGS_EP_MAX_ITEMS && SGS_ENDPOINTS_MAX_DIST == SGS_EP_MAX_DIST && SGS_ENDPOINTS_MAX_ENTRIES == SGS_EP_MAX_ENTRIES &&
              SGS_ENDPOINTS_ITEM_EMPTY == SGS_EP_ITEM_EMPTY && SGS_ENDPOINTS_ITEM_BAD_CELL == SGS_EP_ITEM_BAD_CELL &&
              SGS_ENDPOINTS_ITEM_TOO_LONG == SGS_EP_ITEM_TOO_LONG && SGS_ENDPOINTS_QUERY_TOWARDS == SGS_EP_QUERY_TOWARDS, "the kernels' constants are the header's");

extern "C" {

int sgs_endpoints_tile(void) { return SGS_EP_TILE; }

int64_t sgs_endpoints_work_bytes(int nx, int ny, int n_items) {
    if (nx < 1 || ny < 1 || nx > SGS_EP_MAX_N || ny > SGS_EP_MAX_N || n_items < 1 || n_items > SGS_EP_MAX_ITEMS) return -1;
    return 8 * (int64_t)n_items + (((int64_t)n_items * nx * ny + 7) & ~(int64_t)7);   // the header, and every window the whole grid
}

int sgs_endpoints(sgs_ctx* ctx, const void* src, const sgs_endpoints_params* p, const uint32_t* item_offsets, const int32_t* item_cells,
                  int n_items, const sgs_endpoints_query* queries, int n_queries, void* work, int64_t work_bytes,
                  sgs_endpoints_item* out_items, sgs_endpoints_answer* out_queries, uint64_t* out_counts, void* hip_stream) {
    if (!ctx) return SGS_ERR_INVALID;
    const char* who = "sgs_endpoints"; const Args a = {ctx, who};
    SGS_TRY(a.non_null(src, "src", p, "params", item_offsets, "item_offsets", item_cells, "item_cells", work, "work", out_items, "out_items",
                       out_counts, "out_counts"));
    if (n_queries < 0 || n_queries > SGS_ENDPOINTS_MAX_QUERIES) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_queries = %d (0 <= n_queries <= %d)", who, n_queries, SGS_ENDPOINTS_MAX_QUERIES);
    if (n_queries > 0) SGS_TRY(a.non_null(queries, "queries", out_queries, "out_queries"));
    if (n_items < 1 || n_items > SGS_EP_MAX_ITEMS) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: n_items = %d (1 <= n_items <= %d)", who, n_items, SGS_EP_MAX_ITEMS);
    SGS_TRY(a.grid_within(p->nx, p->ny, SGS_EP_MAX_N));
    if (p->source != SGS_ENDPOINTS_SRC_MASK8 && p->source != SGS_ENDPOINTS_SRC_D2) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown source %d", who, (int)p->source);
    if (p->max_dist < 0 || p->max_dist > SGS_EP_MAX_DIST) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: max_dist = %d (0 <= max_dist <= %d)", who, (int)p->max_dist, SGS_EP_MAX_DIST);
    if (p->source == SGS_ENDPOINTS_SRC_MASK8 && p->max_d2 != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: max_d2 = %u with a mask", who, (unsigned)p->max_d2);
    if (p->flags != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->reserved != 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: reserved = %d", who, (int)p->reserved);
    if (work_bytes < 0) SGS_FAIL(ctx, SGS_ERR_INVALID, "%s: work_bytes = %lld", who, (long long)work_bytes);
    SGS_TRY(a.aligned(4, item_offsets, "item_offsets", item_cells, "item_cells", queries, "queries", out_queries, "out_queries"));
    if (p->source == SGS_ENDPOINTS_SRC_D2) SGS_TRY(a.aligned(4, src, "src"));        // a mask is read byte by byte
    SGS_TRY(a.aligned(8, work, "work", out_items, "out_items", out_counts, "out_counts"));
    SGS_TRY(a.disjoint(work, (uint64_t)work_bytes, "work", out_items, sizeof(sgs_endpoints_item) * (uint64_t)n_items, "out_items"));
    SGS_TRY(a.disjoint(work, (uint64_t)work_bytes, "work", out_queries, sizeof(sgs_endpoints_answer) * (uint64_t)n_queries, "out_queries"));
    SGS_TRY(a.disjoint(work, (uint64_t)work_bytes, "work", out_counts, 32, "out_counts"));
    SGS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int64_t header = 8 * (int64_t)n_items;
    sgs::EpJob J;
    J.src = src; J.offsets = item_offsets; J.cells = item_cells; J.queries = reinterpret_cast<const sgs::EpQuery*>(queries);
    J.win_off = static_cast<unsigned long long*>(work); J.field = static_cast<unsigned char*>(work) + header;
    J.items = reinterpret_cast<sgs::EpItem*>(out_items); J.answers = reinterpret_cast<sgs::EpAnswer*>(out_queries);
    J.counts = reinterpret_cast<unsigned long long*>(out_counts);
    J.work_bytes = (unsigned long long)work_bytes; J.has_header = work_bytes >= header;
    J.nx = p->nx; J.ny = p->ny; J.n_items = n_items; J.n_queries = n_queries; J.kind = p->source; J.max_dist = p->max_dist; J.max_d2 = p->max_d2;
    const dim3 threads(SGS_EP_THREADS);
    const unsigned items = (unsigned)n_items;
    // What a window can hold at most: the grid.  The kernels stride over what it does hold.
    const auto blocks = [](int64_t units, int64_t per_block, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((units + per_block - 1) / per_block, cap)); };
    const int64_t segs = (p->nx + SGS_EP_TILE - 1) / SGS_EP_TILE;
    hipLaunchKernelGGL(sgs::k_ep_items, dim3(items), threads, 0, st, J);
    hipLaunchKernelGGL(sgs::k_ep_scan, dim3(1), threads, 0, st, J);
    if (work_bytes > header) {                                                       // otherwise no window fits and the field kernels would return at once
        hipLaunchKernelGGL(sgs::k_ep_clear, dim3(blocks((work_bytes - header) / 8, SGS_EP_THREADS * 4, 4096)), threads, 0, st, J);
        hipLaunchKernelGGL(sgs::k_ep_mark, dim3(blocks(SGS_EP_MAX_ENTRIES, SGS_EP_THREADS, 16), items), threads, 0, st, J);
        hipLaunchKernelGGL(sgs::k_ep_boundary, dim3(blocks(segs * p->ny, SGS_EP_WAVES, 32), items), threads, 0, st, J);
        hipLaunchKernelGGL(sgs::k_ep_rows, dim3(blocks(p->ny, SGS_EP_WAVES, 32), items), threads, 0, st, J);
        hipLaunchKernelGGL(sgs::k_ep_cols, dim3(blocks(p->nx, SGS_EP_THREADS, 16), items), threads, 0, st, J);
    }
    if (n_queries > 0) hipLaunchKernelGGL(sgs::k_ep_query, dim3((unsigned)n_queries), threads, 0, st, J);
    SGS_HIP(ctx, hipGetLastError());
    return SGS_OK;
}

}  // extern "C"
