/* sage_gs.h — C ABI of libsage_gs.so, the MI355X-native 3D-Gaussian-splatting scene renderer that
 * stands in for the Isaac Sim render step of Galery23/SAGE-3D_Official.
 *
 * The reference has NO FFI for this path: it drives a closed renderer through the Isaac Sim Camera
 * protocol.  Each entry point below names the reference call site(s) it replaces (paths relative to
 * the reference root).  Signatures are plain C: pointers, sizes, PODs; no C++ or
 * torch types, no exceptions.  Every function returns 0 on success or a negative sgs_status; the
 * message of the last failure on a context is available from sgs_last_error().
 *
 * Ownership: the caller owns every input and output buffer.  The library owns only its per-context
 * scratch (freed by sgs_destroy) and the re-laid-out scene copy (freed by sgs_scene_free).
 * Threading: a context is bound to one HIP device and is not re-entrant; work is stream-ordered on
 * the stream passed in (NULL = the device's default stream).  Distinct contexts may be used from
 * distinct threads/processes (one process per GPU is the intended deployment).
 *
 * There is deliberately no CPU backend behind this ABI: sgs_create(…, SGS_BACKEND_CPU, …) fails
 * with SGS_ERR_BACKEND.  The CPU restatement lives in oracle/ and is test infrastructure only.
 */
#ifndef SAGE_GS_H
#define SAGE_GS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGS_VERSION 114            /* major*100 + minor.  The version changes whenever a struct below changes size or meaning
                                    * (100 -> 101: sgs_stats grew d_super; 110: round-4 entry points; 111: sgs_stats grew n_deep_windows, sgs_compressed_scene.reserved_ became sh_decode; 112: SGS_FLAG_NO_DEEP; sgs_set_tuning,
                                    * SGS_BUF_SCENE_SH; 113: fine tiles — sgs_tuning grew fine_tile_pixels, SGS_FLAG_NO_FINE_TILES;
                                    * 114: sgs_tuning grew fine_tile_growth): a caller compiled against
                                    * another header MUST refuse to run — check sgs_version() == SGS_VERSION and, for bindings
                                    * that restate the structs by hand (ctypes, cgo), sgs_struct_sizes() — before the first call
                                    * that takes a struct.  The library writes whole structs (sgs_stats arrays with ITS stride). */
#define SGS_TILE 16                /* 16x16-pixel tiles (BASELINE.json north_star) */

typedef enum sgs_status {
    SGS_OK = 0,
    SGS_ERR_INVALID = -1,          /* bad argument */
    SGS_ERR_HIP = -2,              /* a HIP runtime call failed */
    SGS_ERR_OOM = -3,              /* device allocation failed */
    SGS_ERR_OVERFLOW = -4,         /* more (Gaussian,tile) records than the record capacity */
    SGS_ERR_BACKEND = -5           /* backend not available (only SGS_BACKEND_HIP exists) */
} sgs_status;

enum { SGS_BACKEND_CPU = 0, SGS_BACKEND_HIP = 1 };

/* sgs_config.flags */
enum {
    SGS_FLAG_ASYNC  = 1u << 0,     /* do not synchronise the stream; collect with sgs_frame_sync() */
    SGS_FLAG_TIMING = 1u << 1,     /* bracket every stage with HIP events (fills sgs_stats.ms[]) */
    SGS_FLAG_STATS  = 1u << 2,     /* also count D_f (records consumed by the composite): OFF by default — the per-pixel
                                      bookkeeping costs a sweep ~6 %; sgs_stats.d_fetched and bytes[RENDER]'s D_f term are 0 without it */
    SGS_FLAG_FULL_SORT = 1u << 3,  /* tests: order every queue completely (the production path sorts
                                      lazily and stops once a tile's pixels have all terminated) */
    SGS_FLAG_LOOSE_CULL = 1u << 5, /* tests: bin every splat over S3's reference rect (the production path bins the part of it
                                    * the alpha >= alpha_min ellipse can reach) and decide the 8x8 quadrants inside a tile from
                                    * the axis-aligned extent only (production: exact ellipse/rectangle test).  D, tile
                                    * offsets and queues then are exactly the reference's; frames must be bit-identical
                                    * either way */
    SGS_FLAG_NO_CHUNK_CULL = 1u << 6, /* tests: project every chunk of the scene (the production path first tests each
                                    * 64-Gaussian chunk's bounding sphere against the frame / the band of tile rows and skips
                                    * the chunks that cannot reach it).  N_v, D, queues and frames must not change */
    SGS_FLAG_NO_DEEP = 1u << 8,    /* tests, A/B: never cull a resident window of a long-lived tile against its live pixels before ranking it
                                    * (DESIGN.md §4.2 item 8).  Frames must not change, bit for bit */
    SGS_FLAG_NO_FINE_TILES = 1u << 9, /* tests, A/B: render this frame through 16x16-pixel tiles whatever its size.  By default a frame of at
                                    * most sgs_tuning.fine_tile_pixels pixels (640x480: the reference's own resolutions, simple_env.py:52,
                                    * run_benchmark.py:1409-1419) is rendered through 8x8-pixel tiles — four times the workgroups, a quarter of the
                                    * queue and of the per-wave splat lists in each: such a frame's time is its slowest tile's — unless its splats are
                                    * so large that the split would more than double the records (sgs_tuning.fine_tile_growth).  WHICH splats reach
                                    * a pixel does not change (S3's rect stays a rect of 16x16-pixel tiles); the tile origin the blend's
                                    * coordinates are relative to does, so the two renderings of a frame agree to fp32 rounding (both within the
                                    * parity tolerance of the oracle), not bit for bit.  SGS_FLAG_FULL_SORT / SGS_FLAG_LOOSE_CULL imply this flag:
                                    * the reference's integer structures are those of 16x16-pixel tiles.  sgs_stats.n_tiles, d_total, d_super,
                                    * max_tile_len and SGS_BUF_TILE_OFFSETS count the tiles actually used.  Version 113 */
    SGS_FLAG_PIPELINED = 1u << 4   /* with SGS_FLAG_ASYNC: the frame may run CONCURRENTLY with other pipelined frames on
                                    * the library's internal streams (a few frames in flight, each with its own
                                    * intermediates: one frame's binning fills the compute units another frame's
                                    * composite leaves idle).  It starts after the work already submitted to `stream`;
                                    * its output is complete — and ordered before later work — only after
                                    * sgs_frame_sync().  sgs_render_batch() always works this way. */
};

/* Pipeline stages, in launch order (index of sgs_stats.ms[] / .bytes[]). */
enum {
    SGS_STAGE_PREPROCESS = 0,      /* S1-S3: SH, EWA projection, AABB, compaction (k_preprocess)          */
    SGS_STAGE_COUNT      = 1,      /* S4a: per-tile counts + exclusive scan (k_bin_count, k_tile_scan)     */
    SGS_STAGE_EMIT       = 2,      /* S4b: duplication into per-tile queues (k_bin_emit)                   */
    SGS_STAGE_RENDER     = 3,      /* S5+S6 fused: lazy per-tile radix depth sort + composite (k_tile_render) */
    SGS_NUM_STAGES       = 4
};

typedef struct sgs_ctx sgs_ctx;        /* opaque */
typedef struct sgs_scene sgs_scene;    /* opaque */

/* Pinhole camera: +Z forward, +X right, +Y down; pixel i covers [i, i+1) so a point on the optical
 * axis lands at pixel coordinate cx - 0.5.  `view` maps MODEL space to camera space (row-major
 * 4x4, RIGID — rows of its 3x3 orthonormal to 1e-5, else SGS_ERR_INVALID at enqueue time: the culling bounds absorb ~1e-4 of
 * non-rigidity and the contract sits an order of magnitude inside that.  A view composed or inverted in fp32 can miss it (a few 1e-6
 * is typical, 1e-5 happens): re-orthonormalise it first, as sage_gs.renderer does for its callers): the asset's model->world transform
 * (Data/template.usda:115-124, rotateXYZ -90,0,0) is folded in by the caller.  Replaces Camera(prim_path, frequency, resolution) + focalLength
 * (simple_env.py:840-844,905; generate_images.py:344-350) and cam.set_world_pose(position,
 * orientation) (simple_env.py:1284; generate_images.py:419-421). */
typedef struct sgs_camera {
    int32_t width, height;
    float fx, fy, cx, cy;
    float view[16];
} sgs_camera;

/* Constants of stages S2-S6; sgs_config_default() fills the canonical values. */
typedef struct sgs_config {
    float near_z;          /* 0.2   cull tz <= near_z                                   */
    float far_z;           /* 1e30  cull tz >  far_z                                    */
    float dilation;        /* 0.3   px^2 added to the 2-D covariance diagonal           */
    float clamp;           /* 1.3   frustum clamp factor on t.xy / t.z                  */
    float alpha_min;       /* 1/255 */
    float alpha_max;       /* 0.99  */
    float t_min;           /* 1e-4  */
    float bg[3];           /* background, linear RGB (Data/template.usda tonemap is NOT applied) */
    int32_t sh_degree;     /* -1 = the scene's degree                                   */
    uint32_t flags;        /* SGS_FLAG_*                                                */
    /* Interleaved tile rows (multi-GPU sharding of one frame): with stride S > 1 the call owns
     * the tile rows phase, phase + S, phase + 2S, ... of the frame — every rank gets the same mix of cheap and
     * expensive rows, whatever the camera looks at.  tile_row_begin/_end then index the OWNED rows (0 .. their
     * count; end < 0 = all of them) and out_rgb is a COMPACT image: owned row k occupies pixel rows
     * [16k, 16k+16) of it.  0 or 1 = the contiguous band [tile_row_begin, tile_row_end) of the frame itself. */
    int32_t tile_row_stride;
    int32_t tile_row_phase;
} sgs_config;

typedef struct sgs_stats {
    int64_t n_gaussians;   /* N                                                          */
    int64_t n_visible;     /* N_v: survivors of culling                                  */
    int64_t d_total;       /* D: records queued (tiles reachable by each splat; S3's rect areas under LOOSE_CULL) */
    int64_t d_fetched;     /* D_f (SGS_FLAG_STATS): records consumed before every pixel of their tile stopped */
    int64_t n_pixels;      /* pixels written by this call                                */
    int32_t n_tiles;       /* tiles in [tile_row_begin, tile_row_end)                    */
    int32_t max_tile_len;  /* longest per-tile queue                                     */
    int32_t n_spill_tiles; /* depth buckets too long for LDS, sorted through HBM         */
    int32_t retries;       /* re-renders after growing the record capacity               */
    float ms[SGS_NUM_STAGES];      /* per-stage GPU time (SGS_FLAG_TIMING), else 0       */
    float ms_total;                /* first launch -> last launch (SGS_FLAG_TIMING)      */
    int64_t bytes[SGS_NUM_STAGES]; /* algorithmic bytes per stage         */
    int64_t d_super;       /* D_s: records in the super-tile queues (level 1 of the binning) */
    int64_t n_deep_windows; /* windows of tile queues that the composite culled against the tile's live pixels BEFORE ranking / staging (tiles that
                            * kept consuming batches; never with SGS_FLAG_STATS) — version 111 */
} sgs_stats;

int sgs_version(void);
/* sizeof(sgs_camera), sizeof(sgs_config), sizeof(sgs_stats) as THIS library was compiled (any pointer may be NULL): what a hand-written
 * binding compares its own struct sizes with at load time (sage_gs/_capi.py does).  The reference has no counterpart (no FFI at all). */
void sgs_struct_sizes(int32_t* camera_bytes, int32_t* config_bytes, int32_t* stats_bytes);
void sgs_config_default(sgs_config* cfg);

/* Replaces SimulationApp({...}) + World() construction (simple_env.py:160-230). */
int sgs_create(int device_id, int backend, sgs_ctx** out);
int sgs_destroy(sgs_ctx* ctx);
const char* sgs_last_error(const sgs_ctx* ctx);    /* ctx may be NULL: last creation error */

/* Record capacity (number of (Gaussian,tile) records the scratch can hold).  Grown automatically
 * by synchronous renders; asynchronous renders fail with SGS_ERR_OVERFLOW instead. */
int sgs_set_record_capacity(sgs_ctx* ctx, int64_t max_records);

/* The library's tuning surface — ALL of it: the library reads nothing from the environment (rounds 2-5 read eight SGS_* variables at
 * sgs_create; four of them — the grids of the binning and projection launches — were settled by A/B runs and are constants now).
 * sgs_tuning_default() fills what the bench runs; sgs_set_tuning() takes effect for the scenes uploaded and the frames issued AFTER it
 * (it completes the frames in flight first).  Frames do not depend on any of these, bit for bit (tests/test_gpu_parity.py).  No
 * counterpart in the reference (one synchronous SimulationApp per process, simple_env.py:163).  Version 112 (113: fine_tile_pixels, 114: fine_tile_growth — the two
 * fields frames DO depend on, to fp32 rounding).  The tiling a frame gets is decided from a probe of the scene drawn by the Gaussians'
 * indices in the caller's order, so neither morton nor the upload path (sgs_scene_upload or sgs_scene_upload_compressed of the same
 * values) changes it; reordering the input still can, to fp32 rounding — as it can reorder the blend of splats whose depths tie (equal
 * depths blend in the order of the caller's indices). */
typedef struct sgs_tuning {
    int32_t lanes;            /* 3  frames in flight for SGS_FLAG_PIPELINED single frames: each lane has its own stream and intermediates (1..16) */
    int32_t group;            /* 8  frames per set of launches in sgs_render_batch* (blockIdx.y selects the frame; 1..8).  The full frames of a
                               *    group are projected by ONE launch that reads what they share of the scene once (r06zb); 8 x 2 against
                               *    4 x 2: -4.5 % per frame on the bench's poses (r06ze) */
    int32_t group_lanes;      /* 2  streams the groups of a batch alternate over (group x group_lanes <= 16) */
    int32_t morton;           /* 1  lay the scene out in Z-order at upload (device radix sort); 0 keeps the caller's order */
    int64_t record_capacity;  /* 16 Mi  (Gaussian, tile) records the queues of a lane hold; an overflowing frame grows them and is rendered again
                               *        (= sgs_set_record_capacity) */
    int64_t fine_tile_pixels; /* 307200 (640x480)  frames of at most this many pixels MAY be rendered through 8x8-pixel tiles, of at most a quarter
                               *        of it through 4x4 (SGS_FLAG_NO_FINE_TILES above); 0 = never.  Version 113 */
    double fine_tile_growth;  /* 2.2  ... and ARE, as long as halving the tiles multiplies the frame's (Gaussian, tile) records by no more than this
                               *        (what a split costs; estimated per frame on the host from 512 Gaussians of the scene, ~6 us).
                               *        Indoor scenes of small splats grow by 1.5-2.0 and gain 20-50 % of a frame; scenes with trained-3DGS
                               *        statistics grow by 2.5-3.5 and would lose 30 %.  >= 16 = whenever the pixel rule allows
                               *        (tests); must be >= 1.  Version 114 */
} sgs_tuning;
void sgs_tuning_default(sgs_tuning* out);
int sgs_set_tuning(sgs_ctx* ctx, const sgs_tuning* tuning);
int sgs_get_tuning(const sgs_ctx* ctx, sgs_tuning* out);

/* Scene load — replaces open_stage(usd_path) resolving /World/gauss (simple_env.py:219;
 * generate_images.py:320-327).  Inputs are fp32, activations already applied:
 *   means[N,3], scales[N,3] (linear), quats[N,4] (w,x,y,z; normalised by the library),
 *   opacities[N] in (0,1), sh[N,(sh_degree+1)^2,3].
 * on_device != 0: the pointers are device pointers on the context's device. */
int sgs_scene_upload(sgs_ctx* ctx, int64_t n, int sh_degree, const float* means, const float* scales,
                     const float* quats, const float* opacities, const float* sh, int on_device,
                     sgs_scene** out);
/* The same, from the PlayCanvas "compressed.ply" payload InteriorGS ships (`3dgs_compressed.ply`, README.md:197-231 of the reference — which
 * converts it back to a standard .ply with @playcanvas/splat-transform and then to USDZ before Isaac Sim can load it): the payload is
 * dequantised ON THE DEVICE while the scene is laid out; the fp32 arrays never exist.  16 bytes per Gaussian instead of 236.
 *   chunks[n_chunks][18]   per 256 Gaussians: min xyz, max xyz, min / max of log(scale) xyz, min rgb, max rgb (0 and 1 when the file has no
 *                          colour range: the chunk element's first 12 or 18 float properties, in file order)
 *   packed[n][4]           the vertex element's uint32 properties packed_position (11-10-11), packed_rotation (2 + 10-10-10), packed_scale
 *                          (11-10-11), packed_color (8-8-8-8), in THIS order
 *   sh[n][3 * ((d+1)^2-1)] the `sh` element's uint8 properties f_rest_*, in file order (channel-major); NULL at degree 0
 * sage_gs/ply.py (read_compressed_payload) produces exactly these from a file.  n_chunks must be ceil(n / 256). */
enum { SGS_SH_DECODE_UNSPECIFIED = 0, SGS_SH_DECODE_LINEAR255 = 1, SGS_SH_DECODE_BIN_CENTRE_ENDS = 2, SGS_SH_DECODE_BIN_CENTRE = 3 };
typedef struct sgs_compressed_scene {
    int64_t n;
    int64_t n_chunks;
    int32_t sh_degree;
    int32_t sh_decode;     /* how an 8-bit SH coefficient v becomes a float — REQUIRED when sh_degree > 0 (version 112: 0 = UNSPECIFIED is refused with
                            * SGS_ERR_INVALID instead of silently meaning "bin centre" as in version 111; ignored at degree 0):
                            *   SGS_SH_DECODE_BIN_CENTRE (3)  v / 32 - 4 + 1 / 64: the centre of the truncation bin trunc((x / 8 + 0.5) * 256) that the
                            *                                 PlayCanvas WRITER (and sage_gs.ply.encode_compressed) puts x into;
                            *   SGS_SH_DECODE_LINEAR255  (1)  v * 8 / 255 - 4: 0 -> -4, 255 -> +4, linear in between — to this builder's recollection what
                            *                                 the PlayCanvas READERS (engine GSplatCompressedData, splat-transform's decompress) apply;
                            *   SGS_SH_DECODE_BIN_CENTRE_ENDS (2)  bin centres, but v = 0 -> -4 and v = 255 -> +4 exactly.
                            * The three differ by at most 1 / 64 per coefficient.  The reference never decodes these bytes itself (README.md:197-231 hands
                            * the file to @playcanvas/splat-transform, un-vendored, unpinned and not installable here), so which of them that tool
                            * applies cannot be pinned from this container — which is why there is no default: say which one your converter uses
                            * (tests/golden/compressed_ply_kat.json lists every byte's value under all three). */
    const float* chunks;
    const uint32_t* packed;
    const uint8_t* sh;
} sgs_compressed_scene;
int sgs_scene_upload_compressed(sgs_ctx* ctx, const sgs_compressed_scene* z, int on_device, sgs_scene** out);
int sgs_scene_free(sgs_ctx* ctx, sgs_scene* scene);

/* One frame — replaces world.step(render=True) x2..5 + cam.get_rgba() (simple_env.py:1368-1380;
 * generate_images.py:425-428).  Renders the tile rows [tile_row_begin, tile_row_end) of the frame
 * (tile_row_end < 0: all rows) into out_rgb, a DEVICE buffer of height*width*3 floats (row-major,
 * RGB interleaved); rows outside the range are left untouched.  stats may be NULL. */
int sgs_render(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config* cfg,
               int tile_row_begin, int tile_row_end, float* out_rgb, sgs_stats* stats,
               void* hip_stream);

/* As sgs_render, plus out_aux: a DEVICE buffer of height*width*2 floats — per pixel the expected view
 * depth sum_i T_i alpha_i z_i (metres along the optical axis) and the coverage 1 - T_final.  This is the
 * natural Gaussian-scene counterpart of the reference's depth channel, which renders the depth of the
 * collision mesh instead (simple_env.py:1395-1589: get_depth, clipped to [0.1, 6.5] m).
 * out_aux is always the FULL frame's buffer: a band [tile_row_begin, tile_row_end) writes its own pixel rows of it and leaves the
 * others alone, as in out_rgb.  There is no compact form: out_aux != NULL with cfg->tile_row_stride > 1 is refused with
 * SGS_ERR_INVALID (render the interleaved rows' colours with sgs_render; depth / coverage by bands). */
int sgs_render_rgbd(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cam, const sgs_config* cfg,
                    int tile_row_begin, int tile_row_end, float* out_rgb, float* out_aux,
                    sgs_stats* stats, void* hip_stream);

/* B frames of one scene, back to back, one synchronisation at the end — the frame loop of
 * generate_images.py:408-436.  out_rgb holds B consecutive frames; stats (nullable) B entries.  (With
 * cfg->tile_row_stride > 1 every frame still has a height*width*3 slot; its compact image starts at the slot.)
 * The frames are issued in groups of up to sgs_tuning.group CONSECUTIVE cameras; the frames of a group are projected by one launch
 * that reads what they both see of the scene once — pass a trajectory's cameras in path order (neighbours share nearly everything:
 * 7-10 % per frame; unrelated views: 2-5 %).  Every frame equals the frame sgs_render() renders, bit for bit. */
int sgs_render_batch(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cams, int n_cams,
                     const sgs_config* cfg, int tile_row_begin, int tile_row_end, float* out_rgb,
                     sgs_stats* stats, void* hip_stream);

/* As sgs_render_batch, with the frames' outputs `frame_stride` FLOATS apart: frame i is stored as if out_rgb + i *
 * frame_stride were the address of its pixel (0,0).  This is what a rank of a tile-row-sharded sweep uses — every
 * frame's band of rows goes to its own slab (sage_gs/dist.py) — and what keeps the host out of the way there: the whole
 * batch is one call, and the library forks its internal streams, clears and collects the frames' status words and waits
 * for completion once per batch instead of once per frame. */
int sgs_render_batch_strided(sgs_ctx* ctx, const sgs_scene* scene, const sgs_camera* cams, int n_cams,
                             const sgs_config* cfg, int tile_row_begin, int tile_row_end, float* out_rgb,
                             int64_t frame_stride, sgs_stats* stats, void* hip_stream);

/* Completes frames issued with SGS_FLAG_ASYNC: waits for the stream of the MOST RECENT frame and for every
 * pipelined frame in flight, checks the status of every frame issued since the previous synchronisation and
 * reports the statistics of the most recent one.  A caller that spreads asynchronous, non-pipelined frames over
 * several streams of its own must synchronise the earlier streams itself (one stream per context is the
 * intended use; pipelined frames are the library's way to overlap frames). */
int sgs_frame_sync(sgs_ctx* ctx, sgs_stats* stats);

/* Records queued per FRAME tile row (out[r], r < n_rows <= 4096), summed over every frame rendered since the last call with
 * reset != 0 — each frame adds the rows it rendered (its band).  This is the per-row cost from which cost-balanced
 * tile-row bands are cut (SURVEY.md §8e "optional cost-balanced ranges from the previous frame's per-row D"); the
 * reference has no counterpart (it shards by scene only, generate_images.py:136-139).  Covers the frames that have
 * been completed (synchronous frames, or asynchronous ones after sgs_frame_sync); frames still in flight may be
 * counted partly. */
int sgs_row_records(sgs_ctx* ctx, int64_t* out, int n_rows, int reset);

/* fp32 RGB -> uint8 RGBA (alpha 255), the shape cam.get_rgba() returns (simple_env.py:1380-1386;
 * generate_images.py:428-431).  `rgb` is a device buffer; `rgba` is a device buffer or PINNED host memory the device can address
 * (hipHostMalloc / a torch pin_memory tensor: the kernel then writes the host buffer itself, over the link — for a single frame a
 * caller is waiting for that is 25-30 us shorter than a device buffer plus a copy, sage_gs.Renderer.render_rgba8_host). */
int sgs_pack_rgba8(sgs_ctx* ctx, const float* rgb, uint8_t* rgba, int width, int height,
                   void* hip_stream);

/* Test hook: copy an intermediate buffer of the LAST synchronous frame to host memory.
 * Returns the number of bytes the buffer holds (copying at most `bytes`), or a negative status. */
enum {
    SGS_BUF_TILE_OFFSETS = 0,      /* uint32[T+1]                                                */
    SGS_BUF_SORTED_SLOTS = 1,      /* uint32[D]    per-tile queues in (depth, index) order — complete only with SGS_FLAG_FULL_SORT */
    SGS_BUF_SLOT_IDS     = 2,      /* uint32[S]    slot i holds Gaussian i: i if live this frame, 0xFFFFFFFF if culled; S = ceil(N/64)*64 */
    SGS_BUF_CHUNK_SKIPPED = 4,     /* uint8[ceil(N/64)]  1 = the 64-Gaussian chunk (in layout order) was skipped by its bounds */
    SGS_BUF_SPLATS       = 3,      /* S x 12 words: x,y,conic a,b | c,opacity,r,g | b,depth bits,rect01,rect23 (dead = 0) */
    SGS_BUF_SCENE_GEOM   = 5,      /* float[N][11] of the LAST RENDERED scene as the device holds it, by original index: mean xyz, opacity, scale xyz,
                                    * quaternion wxyz (as uploaded / as dequantised from a compressed payload) */
    SGS_BUF_SCENE_SH     = 6,      /* float[N][3 (d+1)^2] of the LAST RENDERED scene, by original index, [coefficient][channel]: the SH coefficients the
                                    * projection kernel evaluates — the fp32 rows as uploaded, or (a scene uploaded from the compressed payload, which
                                    * keeps its 8-bit coefficients as bytes in HBM) those bytes dequantised exactly as the kernel does */
    SGS_BUF_SCENE_PERM   = 7,      /* uint32[N] of the LAST RENDERED scene: layout position p holds the Gaussian of original index perm[p] — the
                                    * Z-order the upload's radix sort made; the identity when the scene was not sorted (sgs_tuning.morton = 0,
                                    * or N <= 64).  Read from the host copy the upload keeps: no per-frame work */
    SGS_BUF_CHUNK_BOUNDS = 8       /* float[ceil(N/64)][8] of the LAST RENDERED scene, in layout order: per 64-Gaussian chunk the bounding sphere
                                    * of its means (cx, cy, cz, R; R = +inf: never skipped) and (s_max, 0, 0, 0), its largest scale — what the
                                    * projection kernel tests a chunk against before it loads it.  Both are new VALUES of `what`, no struct
                                    * changes: SGS_VERSION stays 114 */
};
int64_t sgs_debug_read(sgs_ctx* ctx, int what, void* host_dst, int64_t bytes);

/* ---- Collision-mesh depth — replaces SimpleVLNEnv.get_depth() (simple_env.py:1395-1589): the reference makes /World/scene_collision
 * visible, renders Isaac Sim's `distance_to_image_plane` of the COLLISION MESH and clips it to [0.1, 6.5] m.  The mesh is the payload
 * `{scene_id}_collision.usd` of the template's scene_collision prim (Data/template.usda:156-165).  Synchronous only; no new struct.
 *
 *   Rays     pixel (x, y) is sampled along r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1) in camera space — the pixel centres the splat
 *            path uses (it projects a point to fx x / z + cx - 0.5 and samples pixel i at coordinate i).
 *   Output   out_depth[y * W + x] = the camera-space z of the NEAREST hit on any triangle among hits with near_z < z <= far_z (cfg, or
 *            sgs_config_default's 0.2 / 1e30), both faces counting (collision meshes are not reliably wound); +inf where nothing is hit.
 *            This is `distance_to_image_plane` (z along the optical axis), not the distance along the ray.  A DEVICE buffer of H*W floats.
 *   Camera   sgs_camera.view maps MESH MODEL space to camera space and must be rigid (as for sgs_render; a model scale is baked into the
 *            vertices by the caller — sage_gs.Renderer.upload_mesh does).  All cameras of one call share one resolution.
 *   Refused  with SGS_ERR_INVALID: cfg->tile_row_stride > 1, SGS_FLAG_ASYNC / SGS_FLAG_PIPELINED, a non-rigid view; at upload, triangle
 *            indices outside [0, n_vertices) and non-finite vertices — checked ON THE DEVICE through a status word (the arrays may be
 *            device pointers, on_device != 0), so the upload synchronises once.
 *   Records  the mesh path owns its record buffer: 4 bytes per (triangle, 16x16-pixel tile) record, 4 Mi records (16 MiB) to start
 *            with (sgs_mesh_set_record_capacity); a frame that needs more grows it and is rendered again (sgs_stats.retries).  Besides it,
 *            per (triangle, frame of a group of up to 8 frames) 72 bytes of setup records + 4 bytes, and 8 bytes per tile and frame.
 *   stats    nullable (n_cams entries for the batch): n_visible (triangles that survive culling and reach a tile of the band), d_total
 *            (records), n_tiles, max_tile_len, n_pixels, retries, and ms_total under SGS_FLAG_TIMING (a batch: its group's time / frames
 *            in the group); every other field is 0.
 *   Exact    the value of a pixel is a minimum over the triangles listed for its tile, so it does not depend on the order of the records:
 *            every frame is bit-identical whether rendered alone or in a batch, as a band of tile rows or as the full frame, and under
 *            any permutation of the triangles.  Watertight: two triangles that share an edge (the same two vertex indices) leave no pixel
 *            between them (sage-3d_official_amd/csrc/sgs_mesh.h says how). */
typedef struct sgs_mesh sgs_mesh;      /* opaque */
/* vertices float[V][3], triangles int32[F][3] (host pointers, or device pointers on the context's device when on_device != 0): copied. */
int sgs_mesh_upload(sgs_ctx* ctx, int64_t n_vertices, const float* vertices, int64_t n_triangles, const int32_t* triangles,
                    int on_device, sgs_mesh** out);
int sgs_mesh_free(sgs_ctx* ctx, sgs_mesh* mesh);
/* Record buffer of the mesh path, in records (1 .. 2^32 - 16): takes effect at the next mesh frame. */
int sgs_mesh_set_record_capacity(sgs_ctx* ctx, int64_t max_records);
/* One frame: the tile rows [tile_row_begin, tile_row_end) (end < 0: all) of out_depth (H*W floats); other rows are left untouched. */
int sgs_render_mesh_depth(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cam, const sgs_config* cfg,
                          int tile_row_begin, int tile_row_end, float* out_depth, sgs_stats* stats, void* hip_stream);
/* n_cams whole frames, out_depth[B][H][W]; issued in groups of up to 8 frames per set of launches. */
int sgs_render_mesh_depth_batch(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cams, int n_cams,
                                const sgs_config* cfg, float* out_depth, sgs_stats* stats, void* hip_stream);

/* ---- Collision-mesh object ids — which object each pixel shows: the label of the triangle whose hit sgs_render_mesh_depth* reports.
 * The reference never reads such a channel (its ObjectNav / object-based success decide on the 2-D map only): this is THIS PROJECT'S
 * definition, checked against the fp64 ray caster that checks the depth (tests/mesh_id_ref.py).  No new struct, no new version.
 *
 *   Labels   one int32 per triangle, 0 <= label <= INT32_MAX - 1 (sgs_mesh_set_labels; typically the index of the `def Mesh` prim the
 *            triangle came from).  A mesh without labels uses the triangle's index.
 *   Frames   exactly as sgs_render_mesh_depth*: the same rays, near / far rule, both faces, refusals, record buffer and its growth, stats,
 *            synchronous only; a band of tile rows leaves the other rows of BOTH outputs untouched.  The same five launches per group of
 *            up to 8 frames, the last one k_mesh_ids in place of k_mesh_depth; 4 more bytes are gathered per record, 4 more written per pixel.
 *   Value    out_id[y * W + x] (a DEVICE buffer of H*W int32) = the label of the hit the depth frame reports: among the hits with
 *            near_z < z <= far_z the one with the least fp32 z, and among hits whose z is bit-equal the LEAST LABEL; SGS_ID_NONE where
 *            nothing is hit.  Both kernels decide a hit with the same source (mesh_hit, csrc/sgs_mesh.h).
 *   Depth    out_depth (nullable) is bit-identical to what sgs_render_mesh_depth* writes for the same call.
 *   Exact    a pixel's value is the minimum of the pair (z, label), in that order, over the triangles listed for its tile, so it does not
 *            depend on the order of the records: a frame's ids are bit-identical alone or in a batch, as a band or as the full frame, and
 *            under any permutation of the triangles that carries the labels along.  With the default labels (the triangle's index) the last
 *            guarantee does not hold: a permutation renames the triangles. */
#define SGS_ID_NONE (-1)
/* labels int32[n_triangles of the mesh] (a host pointer, or a device pointer when on_device != 0): copied.  NULL restores the default
 * (label = triangle index).  A label outside [0, INT32_MAX - 1] is refused with SGS_ERR_INVALID — checked on the device through the status
 * word, as the upload checks indices — and the mesh's previous labels stay in force.  Synchronises the device. */
int sgs_mesh_set_labels(sgs_ctx* ctx, sgs_mesh* mesh, const int32_t* labels, int on_device);
/* One frame: the tile rows [tile_row_begin, tile_row_end) (end < 0: all) of out_id (H*W int32) and, when given, of out_depth (H*W floats). */
int sgs_render_mesh_ids(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cam, const sgs_config* cfg, int tile_row_begin,
                        int tile_row_end, float* out_depth, int32_t* out_id, sgs_stats* stats, void* hip_stream);
/* n_cams whole frames, out_id[B][H][W] and (nullable) out_depth[B][H][W]. */
int sgs_render_mesh_ids_batch(sgs_ctx* ctx, const sgs_mesh* mesh, const sgs_camera* cams, int n_cams, const sgs_config* cfg,
                              float* out_depth, int32_t* out_id, sgs_stats* stats, void* hip_stream);

/* ---- Baseline JPEG encoding of rendered frames — replaces Image.fromarray(rgb).save(path) of the data-generation loop
 * (generate_images.py:431-432) and the JPEG encoding of every observation the VLM client sends (vlm_client_modular.py:346-351): the file
 * is made on the device from the fp32 frame sgs_render* left there, and only its bytes cross the link.  No new version: no existing
 * struct changes.
 *
 *   Picture  each channel becomes the 8-bit level sgs_pack_rgba8 would write (clamp to [0,1], (unsigned)(x * 255 + 0.5)); YCbCr by the
 *            JFIF full-range BT.601 matrix and the level shift in fp32, never rounded to 8 bits in between; 4:2:0 chroma is the plain
 *            mean of 2x2 pixels; pixels beyond the right / bottom edge of a partial MCU repeat the last column / row; 8x8 DCT-II in fp32;
 *            the Annex K tables of ITU-T T.81 scaled by `quality` with the IJG rule (what libjpeg and PIL write for the same quality);
 *            one rounding per coefficient, F / Q to nearest, halves away from zero; the four Annex K Huffman tables.
 *   File     SOI, JFIF APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS, entropy-coded data with 0xFF stuffing and RSTn markers, EOI: 629 header
 *            bytes.  The restart interval is 48 blocks (8 MCUs of 4:2:0, 16 of 4:4:4): every interval is coded by its own wave.
 *   Exact    the bytes of a frame depend on its pixels and the parameters alone — not on the batch it is issued in or its place there. */
enum { SGS_JPEG_420 = 0, SGS_JPEG_444 = 1 };       /* sgs_jpeg_params.subsampling */
typedef struct sgs_jpeg_params {
    int32_t quality;       /* 1..100 */
    int32_t subsampling;   /* SGS_JPEG_420 (what PIL's save() does by default, hence what the reference's files are) or SGS_JPEG_444 */
    uint32_t flags;        /* none defined: 0 */
    int32_t reserved_;     /* 0 */
} sgs_jpeg_params;
/* quality 95, 4:2:0: what the sweep asks PIL for. */
void sgs_jpeg_params_default(sgs_jpeg_params* params);
/* The most bytes one frame's file can take, or SGS_ERR_INVALID.  Derivation: 629 header bytes + per restart interval of 48 blocks
 * 2 x ceil(48 x 1658 / 8) + 2, where 1658 bits is the longest a block can be coded (DC: 9-bit code + 11 amplitude bits; each of the 63
 * AC coefficients: 16-bit code + 10 amplitude bits), the factor 2 is every byte being 0xFF and stuffed, and + 2 is the RSTn / EOI
 * marker.  No picture comes near it (it is ~2.5x the fp32 frame's third); buffers of this size per frame never overflow. */
int64_t sgs_jpeg_bound(int width, int height, const sgs_jpeg_params* params);
/* Encodes n_frames frames: rgb is a DEVICE buffer, frame i at rgb + i * rgb_frame_stride (floats), height*width*3 floats each as
 * sgs_render* writes them.  The files are laid end to end in `out`: file i is out[out_offsets[i] .. + out_sizes[i]).  out, out_offsets
 * and out_sizes (n_frames entries each) are device buffers or pinned host memory the device can address, as for sgs_pack_rgba8.
 * Stream-ordered and asynchronous: the call does not synchronise (it may, once, when it first sees a parameter set or grows its
 * scratch), so the encode of one chunk runs beside the render of the next; one encode stream at a time per context.
 * Nothing is ever written at or beyond out + out_capacity: a frame whose file would end beyond it is not written at all, offsets and
 * sizes are reported all the same (what a buffer that fits needs), and sgs_jpeg_status says so after the stream has been
 * synchronised; the caller retries with a larger buffer.  The library owns 12 bytes of scratch per restart interval (grown
 * geometrically) and one small table per parameter set, freed by sgs_destroy.
 * SGS_ERR_INVALID: quality outside 1..100, an unknown subsampling, width or height < 1 or > 65535, n_frames < 0, a null buffer, a
 * negative capacity, frames closer together than their size. */
int sgs_encode_jpeg(sgs_ctx* ctx, const float* rgb, int width, int height, int n_frames, int64_t rgb_frame_stride,
                    const sgs_jpeg_params* params, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* out_sizes,
                    void* hip_stream);
/* After the stream of the most recent sgs_encode_jpeg has been synchronised: SGS_OK, or SGS_ERR_OVERFLOW when its files did not fit;
 * bytes_needed (nullable) receives the bytes they take end to end. */
int sgs_jpeg_status(sgs_ctx* ctx, int64_t* bytes_needed);

/* ---- PNG encoding of depth and colour frames — replaces the 16-bit grey PNG the VLM client makes of every depth observation
 * (vlm_client_modular.py:354-365: np.clip(depth, 0, 6.5) * 10000 -> uint16 -> PNG) and the frame_%05d.png sequence of an episode
 * (simple_env.py:2757-2759): the file is made on the device from the fp32 frame, and only its bytes cross the link.  No new version: no
 * existing struct changes.
 *
 *   Samples  SGS_PNG_RGB8: each channel becomes the 8-bit level sgs_pack_rgba8 would write: clamp to [0,1], (unsigned)(x * 255 + 0.5).
 *            SGS_PNG_DEPTH16: v = (uint16) trunc(min(max(d, 0), depth_max) * depth_scale) — one fp32 multiply and a truncation, NumPy's
 *            clip(d, 0, depth_max) * depth_scale -> astype(uint16); +inf (no triangle hit) becomes depth_max, -inf and NaN become 0;
 *            stored big-endian.
 *   File     signature, IHDR (bit depth 8 / colour type 2, or 16 / 0; no interlace), IDAT chunks, IEND, nothing else.  The image is
 *            cut into strips of as many whole rows as fit 16 384 filtered bytes (at least one), one IDAT chunk per strip.  Every row
 *            takes the filter (None, Sub, Up, Average, Paeth) with the least sum of its bytes' absolute values read as signed, ties to
 *            the lowest type; the row above the image is zeros.  A strip is one deflate block — dynamic Huffman codes over literals and
 *            run matches (distance 1, 3..258 bytes), or stored when that is no shorter — followed by an empty stored block, so every
 *            strip ends byte-aligned and matches nothing before itself.  The first chunk carries the zlib header 78 01, the last the
 *            final empty block and the Adler-32.
 *   Exact    the bytes of a frame depend on its samples and the parameters alone — not on the batch it is issued in or its place there. */
enum { SGS_PNG_RGB8 = 0, SGS_PNG_DEPTH16 = 1 };    /* sgs_png_params.format */
typedef struct sgs_png_params {
    int32_t format;        /* SGS_PNG_RGB8: src is fp32 [H,W,3]; SGS_PNG_DEPTH16: src is fp32 [H,W] (metres) */
    float   depth_scale;   /* 10000 (vlm_client_modular.py:356) */
    float   depth_max;     /* 6.5   (vlm_client_modular.py:355) */
    int32_t reserved;      /* 0 */
} sgs_png_params;
/* SGS_PNG_RGB8, 10000, 6.5. */
void sgs_png_params_default(sgs_png_params* params);
/* The most bytes one frame's file can take, or SGS_ERR_INVALID.  Derivation, every strip stored: signature 8 + IHDR 25 + IEND 12 + zlib
 * header 2 + final block 5 + Adler-32 4 = 56, plus per strip 12 bytes of chunk framing, 5 of the stored block's header and 5 of the empty
 * block, plus the filtered bytes, height x (1 + width x bytes per pixel).  A strip that would code longer than stored is stored. */
int64_t sgs_png_bound(int width, int height, const sgs_png_params* params);
/* Encodes n_frames frames: src is a DEVICE buffer, frame i at src + i * src_frame_stride (floats), height*width*3 (RGB8) or height*width
 * (DEPTH16) floats each.  Everything else is as for sgs_encode_jpeg: the files lie end to end in `out`, file i is
 * out[out_offsets[i] .. + out_sizes[i]); out, out_offsets and out_sizes are device buffers or pinned host memory; the call is
 * stream-ordered and does not synchronise (it may, when it grows its scratch); a frame whose file would end beyond out_capacity is not
 * written at all, offsets and sizes are reported all the same, and sgs_png_status says so after the stream has been synchronised.  The
 * library owns one slot of (strip + 16) bytes and 24 bytes per strip, grown geometrically and freed by sgs_destroy.
 * SGS_ERR_INVALID: an unknown format, reserved != 0, a null buffer, n_frames < 0, a negative capacity, width or height < 1, height
 * > 65535, a filtered row longer than 16 384 bytes (width > 5461 for RGB8, > 8191 for DEPTH16), for DEPTH16 depth_scale <= 0, depth_max
 * <= 0 or depth_max * depth_scale > 65535 (in fp32), frames closer together than their size. */
int sgs_encode_png(sgs_ctx* ctx, const float* src, int width, int height, int n_frames, int64_t src_frame_stride,
                   const sgs_png_params* params, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* out_sizes,
                   void* hip_stream);
/* After the stream of the most recent sgs_encode_png has been synchronised: SGS_OK, or SGS_ERR_OVERFLOW when its files did not fit;
 * bytes_needed (nullable) receives the bytes they take end to end. */
int sgs_png_status(sgs_ctx* ctx, int64_t* bytes_needed);

/* ---- Resizing frames — replaces the host-side resize of the benchmark's low-res mode (run_benchmark.py:1409-1419 for RGB,
 * :1441-1451 for depth: cv2.resize or PIL's Image.resize to 320x240) and of odd video frames (simple_env.py:2750): the resized frame is
 * made on the device from the fp32 frame sgs_render* left there and is a frame like any other, so sgs_pack_rgba8, sgs_encode_jpeg and
 * sgs_encode_png take it unchanged.  No new version: no existing struct changes.
 *
 *   Frames   SGS_RESIZE_RGB8: src is fp32 [H,W,3]; each channel first becomes the 8-bit level sgs_pack_rgba8 would write (clamp to
 *            [0,1], (unsigned)(x * 255 + 0.5)), the LEVELS are resampled in integers, and dst is fp32 [h,w,3] holding the fp32
 *            nearest k / 255 of every resampled level k — a value that x * 255 + 0.5 takes back to k, fused or not.
 *            SGS_RESIZE_F32: src is fp32 [H,W], dst fp32 [h,w]; every sample is clipped as it is loaded,
 *            x < clip_lo ? clip_lo : (x > clip_hi ? clip_hi : x) (NaN stays NaN, as with np.clip): the reference's order, clip in
 *            get_depth and then resize, which makes the +inf of a pixel that hit nothing finite before it meets a negative weight.
 *            A window that holds a non-finite sample after the clip gives an unspecified value; every other pixel is unaffected.
 *   Filters  SGS_RESIZE_BICUBIC is PIL's Image.resize(size) at its default resample, bit for bit: separable convolution, per axis
 *            scale = in / out, support = 2 max(scale, 1), centre c = (o + 0.5) scale, taps [max((int)(c - support + 0.5), 0),
 *            min((int)(c + support + 0.5), in)), the cubic with a = -0.5 at (tap - c + 0.5) * (1 / max(scale, 1)), the weights divided by
 *            their sum in tap order, all in fp64 with multiply and add unfused.  RGB8: weights as (int)(w 2^22 +- 0.5), a sample is
 *            clamp((2^21 + sum level kk) >> 22, 0, 255); the horizontal pass runs first and writes 8-bit levels, which the vertical
 *            pass reads.  F32: a sample is (float) sum (double)x w from 0.0 in tap order, unfused; fp32 between the passes.  A pass
 *            whose in-size equals its out-size is skipped, not run with identity weights.
 *            SGS_RESIZE_LINEAR is bilinear at half-pixel centres without a prefilter, clamped at the edges — the sampling cv2
 *            documents for INTER_LINEAR; it is NOT pinned to cv2's bytes but defined exactly: sx = max((2x + 1) W - w, 0),
 *            x0 = sx div 2w, fx = sx mod 2w (x0 >= W - 1: x0 = W - 1, fx = 0), y likewise; RGB8: (sum of the four corners' level
 *            wx wy + 2wh) div 4wh in 64-bit integers, the exact bilinear value rounded half up; F32: the weights fx / 2w and fy / 2h
 *            in fp32, a + (b - a) t horizontally on both rows, then vertically.
 *   Exact    a frame's values depend on its samples and the parameters alone — not on the batch it is issued in or its place there. */
enum { SGS_RESIZE_RGB8 = 0, SGS_RESIZE_F32 = 1 };          /* sgs_resize_params.format */
enum { SGS_RESIZE_BICUBIC = 0, SGS_RESIZE_LINEAR = 1 };    /* sgs_resize_params.filter */
typedef struct sgs_resize_params {
    int32_t format;        /* SGS_RESIZE_RGB8 or SGS_RESIZE_F32 */
    int32_t filter;        /* SGS_RESIZE_BICUBIC or SGS_RESIZE_LINEAR */
    int32_t dst_width;     /* 1..65535 */
    int32_t dst_height;    /* 1..65535 */
    float   clip_lo;       /* SGS_RESIZE_F32: applied to every sample as it is loaded; -inf clips nothing */
    float   clip_hi;       /*                 +inf clips nothing */
    int32_t reserved[2];   /* 0 */
} sgs_resize_params;
/* SGS_RESIZE_RGB8, SGS_RESIZE_BICUBIC, 320 x 240, -inf, +inf. */
void sgs_resize_params_default(sgs_resize_params* params);
/* Resizes n_frames frames of width x height to dst_width x dst_height: frame i is read at src + i * src_frame_stride and written at
 * dst + i * dst_frame_stride (strides in floats).  src is a DEVICE buffer; dst is a device buffer or pinned host memory the device can
 * address, as for sgs_pack_rgba8.  Nothing of dst outside the frames is written.  Stream-ordered and asynchronous: the call does not
 * synchronise (it may, once, when it first sees a pair of sizes or grows its scratch); one resize stream at a time per context.
 * n_frames == 0 is SGS_OK and launches nothing.  The library owns 4 bytes per pixel of the horizontally resized frames (grown
 * geometrically) and one tap table per (in-size, out-size, filter, format) and axis, freed by sgs_destroy.
 * SGS_ERR_INVALID (nothing is ever clamped): an unknown format or filter, reserved != 0, a null buffer with n_frames > 0, n_frames < 0,
 * a size < 1 or > 65535, frames closer together than their size, clip_lo > clip_hi or either of them NaN, src and dst ranges that
 * overlap. */
int sgs_resize(sgs_ctx* ctx, const float* src, int width, int height, int n_frames, int64_t src_frame_stride,
               const sgs_resize_params* params, float* dst, int64_t dst_frame_stride, void* hip_stream);

/* ---- Per-frame visible-object table — which objects a frame shows, how large, where in the picture, how near: one row per label,
 * reduced on the device from the id frame sgs_render_mesh_ids* wrote (and the depth beside it), so that a few dozen rows cross the
 * link where the id frame is 4 bytes a pixel.  Like the id channel this is THIS PROJECT'S definition: the reference reads no such
 * observation (Isaac Sim's camera offers bounding_box_2d_tight beside instance_id_segmentation; nothing of the reference depends on
 * either).  No new version: no existing struct changes.
 *
 *   Rows     row k of a frame describes label k, 0 <= k < n_labels: the pixels of the frame whose id == k.  Every row of every frame
 *            is written, empty ones included; what out_rows held before does not matter.
 *   Counts   out_counts[f][0] = pixels equal to SGS_ID_NONE; out_counts[f][1] = pixels whose id is neither SGS_ID_NONE nor in
 *            [0, n_labels): they are counted there and enter no row, which is not an error here.  For every frame
 *            sum_k n_pixels + counts[0] + counts[1] == height * width.
 *   z_min    a minimum over the fp32 BIT PATTERNS of the label's depth samples, read as uint32, among those <= 0x7F800000: +0,
 *            denormals, positive finite values and +inf enter; negative numbers, -0 and NaNs do not (their pixels still count in
 *            every other field).  For the frames of the mesh path (positive z, +inf where nothing is hit) it is the plain minimum.
 *   Exact    every field is an integer count, sum, minimum or maximum, so a frame's table depends on its pixels and n_labels alone —
 *            not on the batch it is issued in, its place there, frame_stride, or how the kernel splits the frame: it equals the table
 *            of the frame alone, bit for bit.  Kernels: sage-3d_official_amd/csrc/sgs_objects.h. */
typedef struct sgs_object_row {      /* 40 bytes, 8-byte aligned; row k of a frame's table describes label k */
    uint32_t n_pixels;               /* pixels of the frame whose id == k */
    int32_t  x_min, y_min;           /* least x / y among them;            INT32_MAX in an empty row */
    int32_t  x_end, y_end;           /* greatest x / y among them, plus 1; 0 in an empty row         */
    float    z_min;                  /* least depth among them (rule above); +inf in an empty row, and everywhere when depth == NULL */
    uint64_t sum_x, sum_y;           /* sum of x, sum of y over them (centroid = sum / n_pixels); 0 in an empty row */
} sgs_object_row;
/* n_frames frames of height x width: frame f's ids at ids + f * frame_stride and (depth nullable) its depth at depth + f * frame_stride
 * (elements; the same stride for both), laid out as sgs_render_mesh_ids_batch writes them — but any int32 frame is accepted.  ids and
 * depth are DEVICE buffers; out_rows [n_frames][n_labels] and out_counts [n_frames][2] are device buffers too: the kernels update them
 * with integer atomics (add, unsigned min / max), which a link to pinned host memory need not carry, so unlike sgs_pack_rgba8's output
 * they must not be host memory.  Stream-ordered and asynchronous, as the encoders are: the call never synchronises, owns no scratch and
 * leaves none behind.  Two launches: a clear of the table and one reduction over frames x regions of a frame.
 * SGS_ERR_INVALID, before anything is enqueued or written: null ids, out_rows or out_counts; n_frames < 1; height < 1 or width < 1;
 * height * width > 2^31 - 1; frame_stride < height * width; n_labels < 1; out_rows not 8-byte aligned (sum_x and sum_y are updated
 * with 64-bit atomics); ids, depth (when given) or out_counts not 4-byte aligned.  The message names the argument. */
int sgs_object_table(sgs_ctx* ctx, const int32_t* ids, const float* depth, int n_frames, int height, int width, int64_t frame_stride,
                     int32_t n_labels, sgs_object_row* out_rows, uint32_t* out_counts, void* hip_stream);

/* ---- Image similarity — windowed SSIM and squared error of rendered frames against a target picture, reduced on the device to one
 * 64-byte row per frame.  The reference names the measure and implements none: ImgNav's success is "current view similar to target
 * image" (task_types.py:183-208) and the function behind it returns a placeholder.  So, like the id channel and the object table,
 * this is THIS PROJECT'S OWN definition.  It works in integers up to one fp64 quotient per window: a frame's row depends on its pixels
 * alone — not on the batch, the frame's place in it, the strides, or how the kernel cuts the frame.  No new version: no existing
 * struct changes.
 *
 *   Levels   every channel of the fp32 frame [H,W,3] first becomes the 8-bit level sgs_pack_rgba8 writes: clamp to [0,1], then
 *            (unsigned)(x * 255 + 0.5).  The target is uint8 [H,W,3], levels already: what a PIL image holds.
 *   Window   11 x 11, separable; 1-D integer taps w = {2, 16, 74, 224, 436, 544, 436, 224, 74, 16, 2}, sum 2048: Wang et al.'s
 *            Gaussian of sigma 1.5 scaled by 2048 and rounded, the centre tap lowered by 1 so that the sum is exact.  A window's
 *            weight is w[j] w[i], total T = 2^22.  Only windows that lie wholly inside the frame count: (H - 10)(W - 10) per channel,
 *            no padding.
 *   Moments  per window and channel, exact integers, x the frame's level and y the target's:
 *            A = sum w x, B = sum w y, Cxx = sum w x^2, Cyy = sum w y^2, Cxy = sum w x y.
 *   Terms    in int64:  n1 = 2 A B + c1               d1 = A^2 + B^2 + c1
 *                       n2 = 2 (T Cxy - A B) + c2     d2 = (T Cxx - A^2) + (T Cyy - B^2) + c2
 *            c1 = 114393189753815 and c2 = 1029538707784335: (0.01 * 255)^2 2^44 and (0.03 * 255)^2 2^44, rounded.  All four stay
 *            below 2^63 (A^2 <= 1.15e18); d1 and d2 are positive, n2 may be negative.
 *   Value    s = ((double)n1 * (double)n2) / ((double)d1 * (double)d2): four int64 -> fp64 conversions, two products, one division,
 *            each rounded once (no sum, so nothing can be contracted); q = (int64)floor(s * 2^30 + 0.5) (s * 2^30 is exact).
 *   Row      ssim_q[c] = sum of q over the windows of channel c; sse[c] = sum of (x - y)^2 over ALL pixels of channel c;
 *            n_windows = (H - 10)(W - 10); n_pixels = H W.  The score is sum_c ssim_q[c] / (3 n_windows 2^30), the mean squared
 *            error sum_c sse[c] / (3 n_pixels) in levels^2: host divisions, left to the caller.  Identical pictures give exactly
 *            n_windows 2^30 per channel.
 *   Kernels  sage-3d_official_amd/csrc/sgs_similarity.h: one workgroup per frame and tile of SGS_SIM_TILE_W x SGS_SIM_TILE_H windows. */
#define SGS_SIM_WINDOW 11
#define SGS_SIM_TILE_W 32
#define SGS_SIM_TILE_H 32
typedef struct sgs_similarity_row {  /* 64 bytes, 8-byte aligned; one per frame */
    int64_t  ssim_q[3];              /* per channel: sum over the windows of q (30 fractional bits) */
    uint64_t sse[3];                 /* per channel: sum over all pixels of (x - y)^2, in levels^2 */
    uint64_t n_windows;              /* (H - 10)(W - 10) */
    uint64_t n_pixels;               /* H W */
} sgs_similarity_row;
/* n_frames frames of width x height: frame f's fp32 [H,W,3] at rgb + f * rgb_frame_stride (floats) against the uint8 [H,W,3] at
 * target + f * target_frame_stride (bytes); target_frame_stride == 0 compares every frame with the one target.  rgb, target and
 * out_rows [n_frames] are DEVICE buffers: the rows are updated with 64-bit atomics, which a link to pinned host memory need not
 * carry.  Every row is written whole; what out_rows held before does not matter.  Stream-ordered and asynchronous: the call never
 * synchronises, owns no scratch and leaves none behind.  A clear of the rows, then one reduction over frames x tiles.
 * SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument: null rgb, target or out_rows;
 * n_frames < 1; width or height below 11 (no window) or above 65535; rgb_frame_stride < 3 width height; a non-zero
 * target_frame_stride < 3 width height; out_rows not 8-byte aligned; rgb not 4-byte aligned. */
int sgs_image_similarity(sgs_ctx* ctx, const float* rgb, int width, int height, int n_frames, int64_t rgb_frame_stride,
                         const uint8_t* target, int64_t target_frame_stride, sgs_similarity_row* out_rows, void* hip_stream);

/* ---- Top-down seen map — what an embodied agent has SEEN: depth frames unprojected on the device and binned by height into a grid of
 * cells, per cell a count of free hits (the floor band) and of occupied hits (the obstacle band); the map module of an exploration or
 * ObjectNav agent that consumes RGB-D, reduced next to the kernel that wrote the depth so that a grid of a few hundred cells a side
 * crosses the link where a 1024 x 768 depth frame is 3 MB.  THIS PROJECT'S OWN definition, like the id channel, the object table and
 * the similarity row: the reference scores NoGoalNav by the 0.5 m cells the agent STOOD in against a guessed total of 400
 * (measures.py:399-437) and keeps no map of what it saw.  No new version: no existing struct changes.
 *
 *   Arithmetic  fp32; every multiply and add is rounded once, in the order written, never contracted; there is no division.
 *   Point    frame f has P = pix_to_map[f], twelve floats: rows k = 0, 1, 2 of (a_k, b_k, c_k), then t_0, t_1, t_2.  Pixel (x, y)
 *            with depth z:  d_k = ((float)x * a_k + (float)y * b_k) + c_k;  p_k = z * d_k + t_k.  p_0, p_1 are map coordinates in
 *            metres, p_2 is the height h.  A caller builds P as map_from_cam . [(1/fx, 0, (0.5 - cx)/fx); (0, 1/fy, (0.5 - cy)/fy);
 *            (0, 0, 1)] — the mesh path's ray through the pixel centre — with t the camera's position in the map; the entry composes
 *            nothing and takes the twelve numbers as given.
 *   Cell     u = (p_0 - origin_x) * inv, v = (p_1 - origin_y) * inv with inv = 1.0f / cell_size computed once on the host.  The point
 *            is inside when u >= 0 && u < (float)nx && v >= 0 && v < (float)ny (NaN is outside); only then i = (int)u, j = (int)v.
 *   Counters every pixel goes to exactly one of four per-frame counters, tested in this order: counts[f][0] z not in
 *            [min_z, max_z]; [1] outside the grid; [2] inside but in neither height band; [3] binned.  They sum to height * width.
 *            out_counts is written whole by every call, whatever it held.
 *   Grid     a binned pixel adds 1 to grid[j][i][0] when free_lo <= h && h <= free_hi (free), else to grid[j][i][1] when
 *            occ_lo < h && h <= occ_hi (occupied): where the bands overlap, free wins.  The grid's total grows by sum_f counts[f][3].
 *   Exact    everything is an integer count: a grid depends on the frames, the matrices and the parameters alone — not on the batch,
 *            the order of the frames, frame_stride, how the kernel cuts a frame, or whether two batches are accumulated by two calls
 *            or by one.  Counts saturate nowhere: a call whose n_frames * height * width exceeds 2^32 - 1 — which could overflow one
 *            cell — is refused; overflow ACROSS accumulating calls (SGS_TOPDOWN_CLEAR not set) is the caller's concern.
 *   Kernels  sage-3d_official_amd/csrc/sgs_topdown.h. */
#define SGS_TOPDOWN_CLEAR 1u         /* sgs_topdown_params.flags: zero the grid before accumulating */
typedef struct sgs_topdown_params {
    int32_t nx, ny;            /* cells; 1 <= nx, ny, and 2*nx*ny <= 2^31 - 1 */
    float   origin_x, origin_y;/* map coordinates of the corner of cell (0,0) */
    float   cell_size;         /* metres, > 0, finite */
    float   min_z, max_z;      /* a sample enters only if min_z <= z && z <= max_z (both false for NaN) */
    float   free_lo, free_hi;  /* height h is "free"     when free_lo <= h && h <= free_hi */
    float   occ_lo,  occ_hi;   /*             "occupied" when occ_lo  <  h && h <= occ_hi; tested only when not free */
    uint32_t flags;            /* SGS_TOPDOWN_CLEAR = 1: zero the grid before accumulating; otherwise add to what it holds */
    int32_t reserved;          /* 0 */
} sgs_topdown_params;
/* 256 x 256 cells of 0.05 m, origin (-6.4, -6.4), z in [0.1, 6.5] (the reference's depth clip, simple_env.py:1578), free
 * [-0.15, 0.15], occupied (0.15, 1.5], SGS_TOPDOWN_CLEAR. */
void sgs_topdown_params_default(sgs_topdown_params* params);
/* n_frames depth frames of width x height, frame f at depth + f * frame_stride (floats), accumulated into ONE grid
 * uint32 [ny][nx][2] (free hits, occupied hits); out_counts is uint32 [n_frames][4].  depth, pix_to_map (float [n_frames][12]), grid
 * and out_counts are DEVICE buffers: the kernels update grid and out_counts with integer atomics, which a link to pinned host memory
 * need not carry.  Stream-ordered and asynchronous: the call never synchronises, owns no scratch and leaves none behind.  A clear
 * (of the counters, and of the grid with SGS_TOPDOWN_CLEAR), then one reduction over frames x regions of a frame per 65535 frames.
 * SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument: null depth, pix_to_map, params,
 * grid or out_counts; n_frames < 1; width < 1 or height < 1; height * width > 2^31 - 1; frame_stride < height * width;
 * n_frames * height * width > 2^32 - 1; nx < 1, ny < 1 or 2 * nx * ny > 2^31 - 1; cell_size, an origin or a band edge not finite;
 * cell_size <= 0; min_z <= max_z not true (NaN included); free_lo > free_hi; occ_lo > occ_hi; unknown flags; reserved != 0; depth,
 * pix_to_map, grid or out_counts not 4-byte aligned. */
int sgs_topdown_map(sgs_ctx* ctx, const float* depth, int width, int height, int n_frames, int64_t frame_stride,
                    const float* pix_to_map, const sgs_topdown_params* params, uint32_t* grid, uint32_t* out_counts, void* hip_stream);
/* The four numbers of a grid uint32 [ny][nx][2], written to out (DEVICE uint64[4]) whatever it held: out[0] cells with
 * occupied >= min_hits; out[1] cells with occupied < min_hits && free >= min_hits; out[2] the sum of free hits; out[3] the sum of
 * occupied hits.  out[0] + out[1] is the number of cells seen.  Stream-ordered and asynchronous, no scratch: a clear followed by one
 * reduction.  SGS_ERR_INVALID, before anything is enqueued or written: null grid or out; nx < 1, ny < 1 or 2 * nx * ny > 2^31 - 1;
 * min_hits < 1; grid not 4-byte aligned; out not 8-byte aligned (it is updated with 64-bit atomics). */
int sgs_topdown_summary(sgs_ctx* ctx, const uint32_t* grid, int nx, int ny, uint32_t min_hits, uint64_t* out, void* hip_stream);

/* ---- Clearance map — where an agent can STAND: the exact squared Euclidean distance transform of obstacle grids, and the position
 * and path checks that look positions up in it.  What the reference's 2-D collision detector does on the host for every motion
 * sub-step and for its collision measures (collision_detector.py:95-132, 191-261): an obstacle grid, SciPy's
 * distance_transform_edt, obstacles grown by the robot radius (dist_m <= robot_radius_m), then positions and ten-sample path
 * segments looked up in the grown grid.  Here the grid stays on the device — a mask, or the seen map sgs_topdown_map wrote —, a batch
 * of maps costs one call, and the growth is a threshold on d2 that the query applies: cell c is inside the grown obstacles iff
 * d2[c] <= max_d2 (sage_gs.clearance.inflation_limit gives the max_d2 of a radius and a scale).  No new version: no existing struct
 * changes.
 *
 *   Source   SGS_CLEARANCE_SRC_MASK8: uint8 [ny][nx], a non-zero byte is an obstacle (the reference's obstacle_map before
 *            inflation).  SGS_CLEARANCE_SRC_TOPDOWN: uint32 [ny][nx][2], the grid of sgs_topdown_map (free hits, occupied hits): a
 *            cell is an obstacle iff occupied >= min_hits, and with SGS_CLEARANCE_UNSEEN_BLOCKS also when occupied < min_hits &&
 *            free < min_hits.  Map k begins k * map_stride ELEMENTS of the source's type (bytes; uint32 words) after map 0.
 *   d2       uint32 [n_maps][ny][nx], dense: d2[j][i] = min over obstacle cells (i', j') of (i - i')^2 + (j - j')^2, in cells^2; 0 on
 *            an obstacle; SGS_CLEARANCE_NONE in every cell of a map without obstacles.  1 <= nx, ny <= 32768, so the largest finite
 *            value, 2 * 32767^2, fits.
 *   Counters out_counts uint32 [n_maps][4], written whole by every call: [0] obstacle cells, [1] cells with 0 < d2 <= max_d2,
 *            [2] cells with max_d2 < d2 < NONE, [3] cells equal to NONE.  They sum to nx * ny.
 *   Exact    all arithmetic is on integers: a map's d2 depends on that map alone — not on the batch, map_stride or how the kernels
 *            cut the map.
 *   Kernels  sage-3d_official_amd/csrc/sgs_clearance.h. */
#define SGS_CLEARANCE_NONE 0xFFFFFFFFu
#define SGS_CLEARANCE_SRC_MASK8 0
#define SGS_CLEARANCE_SRC_TOPDOWN 1
#define SGS_CLEARANCE_UNSEEN_BLOCKS 1u   /* sgs_clearance_params.flags */
typedef struct sgs_clearance_params {    /* 28 bytes */
    int32_t  nx, ny;           /* cells; 1 <= nx, ny <= 32768 */
    int32_t  source;           /* SGS_CLEARANCE_SRC_* */
    uint32_t flags;            /* SGS_CLEARANCE_UNSEEN_BLOCKS (the topdown source only) */
    uint32_t min_hits;         /* the topdown source: >= 1; ignored for a mask */
    uint32_t max_d2;           /* the boundary between out_counts[1] and [2]; d2 does not depend on it */
    int32_t  reserved;         /* 0 */
} sgs_clearance_params;
/* src, work, d2 and out_counts are DEVICE buffers; work is scratch of d2's shape (uint32 [n_maps][ny][nx]) that the caller owns and
 * whose contents before and after the call mean nothing.  Stream-ordered and asynchronous: the call never synchronises, owns no
 * scratch and leaves none behind.  A clear of the counters, a pass over rows and a pass over columns per 65535 maps.
 * SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument: null src, params, work, d2 or
 * out_counts; n_maps < 1; nx or ny outside 1 .. 32768; map_stride shorter than a map (nx * ny bytes; 2 * nx * ny words); an unknown
 * source; unknown flags, or SGS_CLEARANCE_UNSEEN_BLOCKS with a mask; min_hits < 1 with the topdown source; reserved != 0; d2 and
 * work the same buffer or overlapping; work, d2, out_counts or a topdown src not 4-byte aligned. */
int sgs_clearance_map(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_clearance_params* params,
                      uint32_t* work, uint32_t* d2, uint32_t* out_counts, void* hip_stream);

/* The reference's check_collision_3d / check_path_collision_3d for n segments in one launch, against ONE d2 map of nx x ny.
 *
 *   Arithmetic  fp64; every operation is rounded once, in the order written, never contracted; the division is a true division.
 *   Samples  segment (x0, y0) -> (x1, y1) has samples s = 1 .. n_samples: t = (double)s / (double)n_samples,
 *            x = x0 * (1 - t) + x1 * t, y likewise.  With n_samples <= 1 there is one sample, the end point itself, untouched
 *            (check_path_collision_3d:250-251).
 *   Mapping  SGS_CLEARANCE_NEGATE first: x = -x, y = -y; then x = sum_x - x with SGS_CLEARANCE_FLIP_X and y = sum_y - y with
 *            SGS_CLEARANCE_FLIP_Y (forward_position_mapping; sum_x = min_x + max_x, added once on the host).
 *   Pixel    px = rint((x - min_x) / scale), py = rint((y - min_y) / scale); rint rounds ties to even, as Python's round does.
 *   Bounds   inside: 0 <= px < nx and 0 <= py < ny.  Otherwise, when -margin <= px < nx + margin and -margin <= py < ny + margin,
 *            both are clamped to the border; otherwise the sample collides.
 *   Collision  a sample that is inside, or was clamped, collides iff d2[py][px] <= max_d2.
 *   DEPARTURE  a px or py that is not finite (a NaN or infinite coordinate) is outside and COLLIDES.  The reference raises inside a
 *            try there and answers "no collision".
 *   Output   uint32 [n][2]: [0] the index s of the first colliding sample (from 1; 1 for the single-sample form), or 0 for none;
 *            [1] the d2 of the cell the last sample — the end point — landed on after clamping, SGS_CLEARANCE_NONE when it was
 *            outside beyond the margin. */
#define SGS_CLEARANCE_NEGATE 1u          /* sgs_clearance_frame.flags */
#define SGS_CLEARANCE_FLIP_X 2u
#define SGS_CLEARANCE_FLIP_Y 4u
typedef struct sgs_clearance_frame {     /* 64 bytes, 8-byte aligned */
    double   min_x, min_y;     /* the coordinates of pixel (0, 0) */
    double   sum_x, sum_y;     /* min + max of the map's bounds, for the flips */
    double   scale;            /* metres per pixel: finite, > 0 */
    uint32_t flags;            /* SGS_CLEARANCE_NEGATE | FLIP_X | FLIP_Y: the reference's defaults are all three */
    int32_t  margin;           /* pixels of tolerance outside the map, >= 0; the reference's is 2 */
    uint32_t max_d2;           /* a cell collides iff d2 <= max_d2 */
    int32_t  n_samples;        /* the reference's default is 10; <= 1: the end point alone */
    int64_t  reserved;         /* 0 */
} sgs_clearance_frame;
/* d2, segs (double [n][4]: x0, y0, x1, y1) and out are DEVICE buffers.  One launch, stream-ordered and asynchronous.
 * SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument: null d2, segs, frame or out;
 * n < 1; nx or ny outside 1 .. 32768; scale not finite or <= 0; min_x, min_y, sum_x or sum_y not finite; margin < 0; unknown
 * flags; reserved != 0; d2 or out not 4-byte aligned; segs not 8-byte aligned. */
int sgs_clearance_query(sgs_ctx* ctx, const uint32_t* d2, int nx, int ny, const double* segs, int n,
                        const sgs_clearance_frame* frame, uint32_t* out, void* hip_stream);

/* ---- Geodesic distance fields and shortest paths — how FAR one place is from another when walls have to be walked round.  What the
 * reference's trajectory generator plans with one host A* per (start, goal) pair over the grid the clearance map holds
 * (vln_trajectory_generator.py astar_pixel: 8-connected moves, a step costs hypot — 1 or sqrt(2) —, a diagonal move may cut a corner).
 * Here one field from a goal answers every start cell of a map, and a batch of goals on one map is one call.  No new version: no
 * existing struct changes.
 *
 *   Field    for every cell the pair (a, b) = (straight steps, diagonal steps) of the cheapest 8-connected walk to any seed over cells
 *            that are not blocked; its cost is a + b sqrt(2).  A diagonal step needs only its two end cells free.  Seeds hold (0, 0);
 *            blocked and unreachable cells hold SGS_GEODESIC_NONE in both words.
 *   Exact    costs are compared in integers (p = a1 - a2 and q = b2 - b1 by sign, then p^2 against 2 q^2 in 64 bits); sqrt(2) is
 *            irrational, so two different pairs never cost the same: the cheapest pair of a cell is unique even where the walk is
 *            not, the field is the unique fixed point of the relaxation, and its bits do not depend on the schedule, the tiling,
 *            the batch or the number of rounds per call.
 *   Source   SGS_GEODESIC_SRC_MASK8: uint8 [ny][nx], non-zero is blocked.  SGS_GEODESIC_SRC_D2: uint32 [ny][nx], the d2 map
 *            sgs_clearance_map wrote: blocked iff d2 <= max_d2.  Map k begins k * map_stride ELEMENTS after map 0; field f runs on map
 *            field_map[f], so many goals share one map.
 *   Rounds   a round is four launches, one per tile colour (tx & 1, ty & 1) of tiles of sgs_geodesic_tile() cells square: a dirty
 *            tile is solved in LDS with a one-cell halo and marks the neighbours dirty that see a border cell that got smaller.  A
 *            field is final when no tile is dirty; the number of rounds that takes is bounded by the tile crossings of the longest
 *            shortest walk.
 *   Tables   field_map (int32 [n_fields]) and seeds (int32 [n_seeds][3] = field, i, j) are HOST arrays: the call validates them and
 *            carries them to the device in kernel arguments; they may be changed or freed as soon as the call returns.  queries
 *            (int32 [n_queries][3] = field, i, j) is a DEVICE buffer.
 *   Kernels  sage-3d_official_amd/csrc/sgs_geodesic.h. */
#define SGS_GEODESIC_NONE 0xFFFFFFFFu
#define SGS_GEODESIC_SRC_MASK8 0
#define SGS_GEODESIC_SRC_D2 1
#define SGS_GEODESIC_CONTINUE 1u         /* sgs_geodesic_params.flags */
#define SGS_GEODESIC_MAX_N 4096
#define SGS_GEODESIC_MAX_FIELDS 65535
#define SGS_GEODESIC_PATH_MAX_FIELDS 512
typedef struct sgs_geodesic_params {     /* 24 bytes */
    int32_t  nx, ny;           /* cells; 1 <= nx, ny <= 4096 */
    int32_t  source;           /* SGS_GEODESIC_SRC_* */
    uint32_t max_d2;           /* the d2 source: a cell is blocked iff d2 <= max_d2; ignored for a mask */
    uint32_t flags;            /* SGS_GEODESIC_CONTINUE (sgs_geodesic_field only) */
    int32_t  reserved;         /* 0 */
} sgs_geodesic_params;
/* The tile edge of the relaxation, and the uint32 words of `state` for n_fields fields of nx x ny (-1 for arguments the field call
 * would refuse): n_fields * (2 + tiles_x * tiles_y). */
int sgs_geodesic_tile(void);
int64_t sgs_geodesic_state_words(int nx, int ny, int n_fields);
/* src, dist, state and status are DEVICE buffers the caller owns; field_map and seeds are HOST arrays (see Tables).  dist is
 * uint32 [n_fields][ny][nx][2]; state is scratch of sgs_geodesic_state_words words that carries the dirty flags from call to call;
 * status is uint32 [n_fields][2], written whole by every call: [0] tiles still dirty — 0: the field is final —, [1] seeds ignored
 * because their cell is blocked.  Without SGS_GEODESIC_CONTINUE the call sets dist to NONE, places the seeds, marks their tiles dirty
 * and enqueues `rounds` rounds; with it, it takes dist and state as an earlier call with the same arguments left them and enqueues
 * `rounds` more (seeds are validated but not placed again).  Stream-ordered and asynchronous: the call never synchronises.
 * SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument: null src, params, field_map,
 * seeds, dist, state or status; n_maps, n_seeds or rounds < 1; n_fields outside 1 .. 65535; nx or ny outside 1 .. 4096; an unknown
 * source; unknown flags; reserved != 0; map_stride shorter than a map (nx * ny elements); a field_map entry outside 0 .. n_maps - 1;
 * a seed whose field is outside 0 .. n_fields - 1 or whose cell is outside the grid; dist not 8-byte aligned; state, status or a d2
 * src not 4-byte aligned; dist and state overlapping. */
int sgs_geodesic_field(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_geodesic_params* params,
                       const int32_t* field_map, int n_fields, const int32_t* seeds, int n_seeds,
                       uint32_t* dist, uint32_t* state, int rounds, uint32_t* status, void* hip_stream);
/* One thread per query (field, start cell) walks a FINAL field downhill to a seed: at each cell it takes the first neighbour, in the
 * order (di, dj) = (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (-1,1) (1,-1) (1,1), that is in the grid, not blocked, and whose pair is exactly
 * the current pair minus that step.  A path has a + b + 1 cells.  out_cells is int32 [n_queries][max_len][2] = (i, j), the start
 * first; the cells beyond a path's length are left as they were.  out_info is uint32 [n_queries][2]: [0] the cells written, [1] a
 * status: 0 ok; 1 the start is blocked or unreachable (no cell written); 2 the path is longer than max_len and was truncated; 3 the
 * query names no field or no cell of the grid (no cell written); 4 a cell had no downhill neighbour — the field is not final.
 * One launch; field_map travels in its arguments, hence n_fields <= 512 here.  params->flags must be 0.  SGS_ERR_INVALID as for
 * sgs_geodesic_field, and: null dist, queries, out_cells or out_info; n_queries or max_len < 1; dist not 8-byte aligned; queries,
 * out_cells or out_info not 4-byte aligned. */
int sgs_geodesic_path(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_geodesic_params* params,
                      const int32_t* field_map, int n_fields, const uint32_t* dist, const int32_t* queries, int n_queries,
                      int max_len, int32_t* out_cells, uint32_t* out_info, void* hip_stream);

/* ---- Connected regions of a grid — which cells BELONG TOGETHER.  What the reference's semantic_map_builder.py computes with two
 * scipy.ndimage.label calls per scene (the wall pixels of occupancy.png into wall items, its zero pixels into "Unable Area" items), and
 * what reachability on a clearance map is: astar_pixel cuts corners, so two free cells have a path exactly when they lie in one
 * 8-connected region of the free cells.  No new version: no existing struct changes.
 *
 *   Set      a cell is in the set iff lo <= v <= hi, v the cell's value.  SGS_REGIONS_SRC_MASK8: v is a byte of a uint8 [ny][nx] map
 *            (lo = 1, hi = 255: non-zero; lo = hi = wall_value: the reference's occupancy == wall_value).  SGS_REGIONS_SRC_D2: v is a
 *            uint32 word of the map sgs_clearance_map wrote (lo = max_d2 + 1, hi = 0xFFFFFFFF: where the agent can stand).  Map k
 *            begins k * map_stride ELEMENTS after map 0.
 *   Regions  the classes of the set under 8-connectivity (two cells whose coordinates differ by at most 1 in each axis) or
 *            4-connectivity (params.connectivity).  A diagonal pair is connected whatever its two orthogonal cells hold.
 *   Labels   int32 [n_maps][ny][nx], dense: 0 for a cell outside the set, otherwise 1 + the number of regions whose least raster
 *            index j * nx + i is smaller than this region's — scipy.ndimage.label's numbering for both structures.
 *   Rows     out_rows is sgs_region_row [n_maps][max_regions]; row r describes label r + 1.  Regions with a label above max_regions
 *            get no row (their cells still carry the right label); rows past the number of regions are empty rows: area 0, x_min =
 *            y_min = INT32_MAX, x_end = y_end = 0, first = 0xFFFFFFFF, sums 0.  max_regions = 0 with out_rows = NULL: labels only.
 *   Counters out_counts is uint32 [n_maps][4], written whole by every call: [0] regions found (the true number, which may exceed
 *            max_regions), [1] cells in the set, [2] the largest area, [3] the least label that has that area (0: the set is empty).
 *   Exact    everything is an integer minimum, count or sum: a map's output depends on that map and the params alone, not on the
 *            batch, map_stride, the tiling or the schedule.
 *   Kernels  sage-3d_official_amd/csrc/sgs_regions.h: a union-find forest whose parents only ever decrease. */
#define SGS_REGIONS_SRC_MASK8 0
#define SGS_REGIONS_SRC_D2 1
#define SGS_REGIONS_MAX_N 4096
#define SGS_REGIONS_MAX_MAPS 65535
typedef struct sgs_regions_params {      /* 32 bytes */
    int32_t  nx, ny;           /* cells; 1 <= nx, ny <= 4096 */
    int32_t  source;           /* SGS_REGIONS_SRC_* */
    int32_t  connectivity;     /* 4 or 8 */
    uint32_t lo, hi;           /* the set: lo <= v <= hi; hi <= 255 for a mask */
    uint32_t flags;            /* 0 */
    int32_t  reserved;         /* 0 */
} sgs_regions_params;
typedef struct sgs_region_row {          /* 40 bytes, 8-byte aligned */
    uint32_t area;             /* cells */
    int32_t  x_min, y_min;     /* the tight box: x_min <= i < x_end, y_min <= j < y_end */
    int32_t  x_end, y_end;     /* greatest + 1 */
    uint32_t first;            /* the region's least raster index j * nx + i */
    uint64_t sum_x, sum_y;     /* of i and of j over the region's cells */
} sgs_region_row;
/* The tile edge of the local solve, and the uint32 words of `work` for n_maps maps of nx x ny (-1 for arguments the call would
 * refuse). */
int sgs_regions_tile(void);
int64_t sgs_regions_work_words(int nx, int ny, int n_maps);
/* src, work, labels, out_rows and out_counts are DEVICE buffers the caller owns; work is scratch of sgs_regions_work_words words
 * whose contents before and after the call mean nothing.  Stream-ordered and asynchronous: the call never synchronises, owns no
 * scratch and leaves none behind.  SGS_ERR_INVALID, before anything is enqueued or written, with a message that names the argument:
 * null src, params, work, labels or out_counts; null out_rows with max_regions > 0, or max_regions < 0; n_maps outside 1 .. 65535;
 * nx or ny outside 1 .. 4096; an unknown source or connectivity; lo > hi, or hi > 255 with a mask; flags or reserved != 0;
 * map_stride shorter than a map (nx * ny elements); work, labels, out_counts or a d2 src not 4-byte aligned; out_rows not 8-byte
 * aligned; labels and work overlapping. */
int sgs_regions_label(sgs_ctx* ctx, const void* src, int n_maps, int64_t map_stride, const sgs_regions_params* params,
                      uint32_t* work, int32_t* labels, sgs_region_row* out_rows, int32_t max_regions,
                      uint32_t* out_counts, void* hip_stream);

/* ---- Item endpoints — the free cell beside an item ON THE SIDE THAT FACES a target.  What the reference's trajectory generator
 * computes with get_nearest_free_pixel_on_side (a breadth-first search over Python sets, twice per candidate pair of items) before it
 * plans between the two cells, and once per item in build_connectivity_map.  No new version: no existing struct changes.
 *
 *   Items     compressed sparse rows: item k is item_cells[item_offsets[k] .. item_offsets[k + 1]), raster indices y * nx + x,
 *             duplicates allowed (they count in n and in the sums).  Every offset lies inside item_cells: the caller's contract.
 *   Boundary  B: the distinct cells of the item with at least one 4-neighbour that is no cell of the item (outside the grid is none).
 *   Field     d(c): the L1 distance from c to B — the level of the reference's search, which is 4-connected and walks through
 *             obstacles.  Cells with d <= max_dist are examined.
 *   Free      SGS_ENDPOINTS_SRC_MASK8: a byte of the uint8 [ny][nx] map is 0.  SGS_ENDPOINTS_SRC_D2: a word of the map
 *             sgs_clearance_map wrote is > max_d2.
 *   Side      with SGS_ENDPOINTS_QUERY_TOWARDS: (n x - Sx)(n tx - Sx) + (n y - Sy)(n ty - Sy) >= 0 in int64, n the item's entries
 *             and S their sums — the sign of the reference's dot(c - mean, target - mean), exactly.
 *   Answer    among the free cells on that side the least d; (x, y) the one of least raster index at that d; n_at_d how many there
 *             are at that d (1: the reference's answer is forced to be this cell; otherwise the reference returns ONE of them, by the
 *             iteration order of a hash table).  None is -1, -1, -1, 0: nothing within max_dist, a flagged item, item outside
 *             0 .. n_items - 1, a target outside the grid, unknown query flags — checked on the device, no index derived from such a
 *             query is used as an address.
 *   Rows      out_items is one sgs_endpoints_item per item.  Flags: EMPTY (no entry, or offsets that decrease), BAD_CELL (an index
 *             outside 0 .. nx * ny - 1), TOO_LONG (more than 2^19 entries; the slice is not read).  A flagged item has n and flags,
 *             the empty box (x_min = y_min = INT32_MAX, x_end = y_end = 0), cx = cy = -1, and zeroes.  cx, cy: the sums over n
 *             rounded half to even, the reference's instance_centroid_px.  boundary: |B|, valid when the work sufficed.
 *   Counters  out_counts is uint64 [4]: [0] queries answered, [1] queries that answer none, [2] flagged items, [3] the bytes of work
 *             this call needs.  When [3] > work_bytes the item rows (boundary 0) and the counters are written, every query answers
 *             none, and the call still returns SGS_OK: call again with [3] bytes.  sgs_endpoints_work_bytes always suffices.
 *   Kernels   sage-3d_official_amd/csrc/sgs_endpoints.h: a window per item of one byte per cell, a capped L1 distance transform from
 *             wave ballots and two column sweeps, a reduction per query. */
#define SGS_ENDPOINTS_SRC_MASK8 0
#define SGS_ENDPOINTS_SRC_D2 1
#define SGS_ENDPOINTS_MAX_N 4096
#define SGS_ENDPOINTS_MAX_ITEMS 65535
#define SGS_ENDPOINTS_MAX_DIST 63
#define SGS_ENDPOINTS_MAX_ENTRIES (1u << 19)
#define SGS_ENDPOINTS_MAX_QUERIES (1 << 22)
#define SGS_ENDPOINTS_ITEM_EMPTY 1u
#define SGS_ENDPOINTS_ITEM_BAD_CELL 2u
#define SGS_ENDPOINTS_ITEM_TOO_LONG 4u
#define SGS_ENDPOINTS_QUERY_TOWARDS 1u
typedef struct sgs_endpoints_params {    /* 28 bytes */
    int32_t  nx, ny;           /* cells; 1 <= nx, ny <= 4096 */
    int32_t  source;           /* SGS_ENDPOINTS_SRC_* */
    uint32_t max_d2;           /* SRC_D2: free iff d2 > max_d2; 0 with a mask */
    int32_t  max_dist;         /* 0 .. 63; the reference's max_search_dist is 50 */
    uint32_t flags;            /* 0 */
    int32_t  reserved;         /* 0 */
} sgs_endpoints_params;
typedef struct sgs_endpoints_query {     /* 16 bytes */
    int32_t  item;             /* 0 .. n_items - 1 */
    int32_t  tx, ty;           /* the target cell, with SGS_ENDPOINTS_QUERY_TOWARDS */
    uint32_t flags;            /* SGS_ENDPOINTS_QUERY_TOWARDS or 0 */
} sgs_endpoints_query;
typedef struct sgs_endpoints_item {      /* 56 bytes, 8-byte aligned */
    uint32_t n;                /* entries of the list, duplicates included */
    uint32_t flags;            /* SGS_ENDPOINTS_ITEM_* */
    int32_t  x_min, y_min;     /* the tight box: x_min <= x < x_end, y_min <= y < y_end */
    int32_t  x_end, y_end;
    int32_t  cx, cy;           /* the centroid pixel */
    uint32_t boundary;         /* |B| */
    uint32_t reserved;         /* 0 */
    uint64_t sum_x, sum_y;     /* of x and of y over the entries */
} sgs_endpoints_item;
typedef struct sgs_endpoints_answer {    /* 16 bytes */
    int32_t  x, y;             /* the cell, or -1, -1 */
    int32_t  d;                /* its L1 distance to B, or -1 */
    int32_t  n_at_d;           /* candidates at that distance, or 0 */
} sgs_endpoints_answer;
/* The cells of one ballot word (the seams of the field's row pass), and the bytes of `work` that suffice for any n_items items on an
 * nx x ny grid (-1 for arguments the call would refuse). */
int sgs_endpoints_tile(void);
int64_t sgs_endpoints_work_bytes(int nx, int ny, int n_items);
/* All pointers are DEVICE buffers the caller owns; work is scratch whose contents before and after the call mean nothing.
 * Stream-ordered and asynchronous: the call never synchronises and owns no scratch.  SGS_ERR_INVALID, before anything is enqueued or
 * written, with a message that names the argument: null src, params, item_offsets, item_cells, work, out_items or out_counts; null
 * queries or out_queries with n_queries > 0; n_items outside 1 .. 65535; n_queries outside 0 .. 2^22; nx or ny outside 1 .. 4096; an
 * unknown source; max_dist outside 0 .. 63; max_d2 != 0 with a mask; flags or reserved != 0; work_bytes < 0; item_offsets,
 * item_cells, queries, out_queries or a d2 src not 4-byte aligned; work, out_items or out_counts not 8-byte aligned; work overlapping
 * out_items, out_queries or out_counts. */
int sgs_endpoints(sgs_ctx* ctx, const void* src, const sgs_endpoints_params* params, const uint32_t* item_offsets,
                  const int32_t* item_cells, int n_items, const sgs_endpoints_query* queries, int n_queries, void* work,
                  int64_t work_bytes, sgs_endpoints_item* out_items, sgs_endpoints_answer* out_queries, uint64_t* out_counts,
                  void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SAGE_GS_H */
