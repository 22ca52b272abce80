// tests/host_alloc_walk.cpp — the allocation-failure walk of the library's host side (csrc/sgs_api.hip), a stand-alone program built
// against the emulator (tests/hipemu) with AddressSanitizer; tests/test_host_alloc_walk.py builds and runs it.
//
// A fixed script of calls on tiny inputs covers every entry point that allocates.  It runs once with no failure (the reference: every
// return code, every output buffer, the number N of device / pinned allocations it makes).  Then, for every k in [0, N), on a fresh
// context: the k-th allocation of the script is refused — every call must return SGS_OK, SGS_ERR_OOM or, where it was handed what an
// earlier refused call did not make (a null scene or mesh after a failed upload, no frame to read back), SGS_ERR_INVALID — and the
// script runs again on the SAME context, unfailed: every call must return what the reference returned, with byte-identical outputs.
// sgs_create's own allocations are refused one by one before that: it must fail and leave nothing behind.  Exit status 0 = all of that
// held; the sanitizer reports the rest (bad accesses as they happen, leaks at exit).
//
//   host_alloc_walk [first_k [end_k]]      (default: every k)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/sage_gs.h"

namespace {

struct Log {
    std::vector<long long> rc;
    std::vector<std::vector<unsigned char>> out;
    std::vector<int> retried;                   // sgs_stats.retries of the two frames that must overflow and be rendered again
    bool refused = false;                       // a call of this run has returned an error
    int bad = 0;                                // calls whose return code the walk does not accept

    bool verbose = false;                       // (WALK_VERBOSE=1: the unfailed run says what each call returned and when)
    double t0 = omp_get_wtime();

    // invalid_ok: the call was handed something an earlier refused call did not make, so SGS_ERR_INVALID is its right answer
    void call(const char* what, long long r, bool invalid_ok = false, bool may_be_positive = false) {
        rc.push_back(r);
        if (verbose) fprintf(stderr, "walk: %7.3f s  %lld allocations  %s -> %lld\n", omp_get_wtime() - t0, hipemu::alloc_count, what, r);
        const bool ok = r == SGS_OK || (may_be_positive && r > 0);
        if (!ok && r != SGS_ERR_OOM && !(r == SGS_ERR_INVALID && invalid_ok)) {
            fprintf(stderr, "walk: %s returned %lld\n", what, r);
            ++bad;
        }
        if (!ok) refused = true;
    }
    template <class T>
    void keep(const std::vector<T>& v) {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
        out.emplace_back(p, p + v.size() * sizeof(T));
    }
};

unsigned g_seed = 1;
unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65535.0f; }

struct Cloud { int n; std::vector<float> means, scales, quats, opac, sh; };

Cloud make_cloud(int n, unsigned seed) {
    g_seed = seed;
    Cloud c; c.n = n;
    for (int i = 0; i < n; ++i) {
        c.means.insert(c.means.end(), {uni(-1.6f, 1.6f), uni(-1.3f, 1.3f), uni(2.0f, 6.0f)});
        c.scales.insert(c.scales.end(), {uni(0.03f, 0.2f), uni(0.03f, 0.2f), uni(0.03f, 0.2f)});
        float q[4] = {uni(-1.f, 1.f), uni(-1.f, 1.f), uni(-1.f, 1.f), uni(0.2f, 1.f)};
        const float qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (float v : q) c.quats.push_back(v / qn);
        c.opac.push_back(uni(0.2f, 0.95f));
        for (int k = 0; k < 12; ++k) c.sh.push_back(k < 3 ? uni(-1.f, 2.f) : uni(-0.3f, 0.3f));       // degree 1
    }
    return c;
}

sgs_camera make_camera(int w, int h, float dx) {
    sgs_camera c;
    memset(&c, 0, sizeof c);
    c.width = w; c.height = h; c.fx = c.fy = 0.8f * (float)w; c.cx = 0.5f * (float)w; c.cy = 0.5f * (float)h;
    c.view[0] = c.view[5] = c.view[10] = c.view[15] = 1.0f;
    c.view[3] = dx;
    return c;
}

struct Inputs {
    Cloud small_ = make_cloud(200, 11), large = make_cloud(1500, 29);
    // a compressed payload of 200 Gaussians of its own at degree 1 (sgs_kernels.h PackedScene): one chunk of 18 floats, four words and nine bytes each
    std::vector<float> z_chunks;
    std::vector<uint32_t> z_packed;
    std::vector<uint8_t> z_sh;
    // a box of 12 triangles in front of the camera, a label per face
    std::vector<float> verts;
    std::vector<int32_t> tris, labels;
    Inputs() {
        z_chunks = {-1.6f, -1.3f, 2.0f, 1.6f, 1.3f, 6.0f, -3.5f, -3.5f, -3.5f, -1.6f, -1.6f, -1.6f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f};
        g_seed = 47;
        for (int i = 0; i < 200; ++i) {
            for (int k = 0; k < 3; ++k) z_packed.push_back((rnd() << 8) ^ rnd());
            z_packed.push_back(((rnd() << 8) ^ rnd()) | 0x40u);               // (opacity >= 64 / 255)
            for (int k = 0; k < 9; ++k) z_sh.push_back((uint8_t)(112 + rnd() % 32));
        }
        for (int i = 0; i < 8; ++i) verts.insert(verts.end(), {(i & 1) ? 0.7f : -0.6f, (i & 2) ? 0.5f : -0.4f, (i & 4) ? 4.6f : 3.5f});
        const int q[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
        for (int f = 0; f < 6; ++f) {
            tris.insert(tris.end(), {q[f][0], q[f][1], q[f][2], q[f][0], q[f][2], q[f][3]});
            labels.insert(labels.end(), {f, f});
        }
    }
};

int upload(sgs_ctx* ctx, const Cloud& c, sgs_scene** out) {
    return sgs_scene_upload(ctx, c.n, 1, c.means.data(), c.scales.data(), c.quats.data(), c.opac.data(), c.sh.data(), 0, out);
}

// The script.  Every call's return code goes to the log; every output buffer too (pre-filled, so that a refused call leaves a defined one).
void script(sgs_ctx* ctx, const Inputs& in, Log& log) {
    constexpr int W0 = 48, H0 = 40, W1 = 80, H1 = 72;
    sgs_config cfg;
    sgs_config_default(&cfg);
    sgs_stats st;
    auto frame = [&](const char* what, const sgs_scene* sc, int w, int h, uint32_t flags, std::vector<float>* keep_rgb = nullptr) {
        std::vector<float> rgb((size_t)w * h * 3, -1.0f);
        const sgs_camera cam = make_camera(w, h, 0.0f);
        sgs_config c = cfg; c.flags = flags;
        st.retries = -1;
        log.call(what, sgs_render(ctx, sc, &cam, &c, 0, -1, rgb.data(), &st, nullptr), !sc);
        log.keep(rgb);
        if (keep_rgb) *keep_rgb = rgb;
    };

    log.call("sgs_set_record_capacity", sgs_set_record_capacity(ctx, 1 << 15));
    log.call("sgs_mesh_set_record_capacity", sgs_mesh_set_record_capacity(ctx, 4096));
    sgs_scene *small_ = nullptr, *large = nullptr, *packed = nullptr;
    log.call("sgs_scene_upload (200)", upload(ctx, in.small_, &small_));
    log.call("sgs_scene_upload (1500)", upload(ctx, in.large, &large));
    {
        sgs_compressed_scene z;
        memset(&z, 0, sizeof z);
        z.n = 200; z.n_chunks = 1; z.sh_degree = 1; z.sh_decode = SGS_SH_DECODE_BIN_CENTRE;
        z.chunks = in.z_chunks.data(); z.packed = in.z_packed.data(); z.sh = in.z_sh.data();
        log.call("sgs_scene_upload_compressed", sgs_scene_upload_compressed(ctx, &z, 0, &packed));
    }

    // ---- frames: the tile arrays grow (9 -> 25 tiles of 16 pixels), are reused by a smaller frame (9 again) and grow again for the cells
    // of the library's own choice of tiling; the splat arrays likewise (small, large, small)
    std::vector<float> rgb0;
    frame("frame 48x40, 16-pixel tiles", small_, W0, H0, SGS_FLAG_NO_FINE_TILES);
    frame("frame 80x72, 16-pixel tiles", small_, W1, H1, SGS_FLAG_NO_FINE_TILES);
    frame("frame 48x40 after 80x72, 16-pixel tiles", small_, W0, H0, SGS_FLAG_NO_FINE_TILES);
    frame("frame 48x40", small_, W0, H0, 0, &rgb0);
    frame("frame 80x72", small_, W1, H1, 0);
    frame("frame of the larger scene", large, W0, H0, 0);
    frame("frame of the smaller scene after the larger", small_, W0, H0, 0);
    frame("frame of the compressed scene", packed, W0, H0, 0);
    frame("timed frame", small_, W0, H0, SGS_FLAG_TIMING);
    {
        std::vector<float> a((size_t)W0 * H0 * 3, -1.0f), b(a);
        const sgs_camera c0 = make_camera(W0, H0, 0.0f), c1 = make_camera(W0, H0, 0.3f);
        sgs_config c = cfg; c.flags = SGS_FLAG_ASYNC | SGS_FLAG_PIPELINED;
        log.call("pipelined frame 0", sgs_render(ctx, large, &c0, &c, 0, -1, a.data(), nullptr, nullptr), !large);
        log.call("pipelined frame 1", sgs_render(ctx, large, &c1, &c, 0, -1, b.data(), nullptr, nullptr), !large);
        log.call("sgs_frame_sync", sgs_frame_sync(ctx, &st), log.refused);
        log.keep(a); log.keep(b);
    }
    std::vector<float> batch((size_t)3 * W0 * H0 * 3, -1.0f);
    {
        const sgs_camera cams[3] = {make_camera(W0, H0, -0.2f), make_camera(W0, H0, 0.0f), make_camera(W0, H0, 0.2f)};
        log.call("sgs_render_batch of 3", sgs_render_batch(ctx, small_, cams, 3, &cfg, 0, -1, batch.data(), nullptr, nullptr), !small_);
        log.keep(batch);
    }
    log.call("sgs_set_record_capacity (too small)", sgs_set_record_capacity(ctx, 1024));
    frame("frame that overflows and is rendered again", large, W1, H1, 0);
    log.retried.push_back(st.retries);
    frame("reference-binning frame", small_, W0, H0, SGS_FLAG_FULL_SORT | SGS_FLAG_LOOSE_CULL);
    for (int what : {0, 1, 2, 3, 4, 5, 6, 100, 101}) {
        const int64_t have = sgs_debug_read(ctx, what, nullptr, 0);
        log.call("sgs_debug_read (size)", have, log.refused, true);
        std::vector<unsigned char> buf((size_t)(have > 0 ? have : 0), 0);
        log.call("sgs_debug_read", sgs_debug_read(ctx, what, buf.data(), (int64_t)buf.size()), log.refused, true);
        log.keep(buf);
    }
    {
        std::vector<int64_t> rows(8, -1);
        log.call("sgs_row_records", sgs_row_records(ctx, rows.data(), 8, 1));
        log.keep(rows);
    }

    // ---- the collision mesh
    sgs_mesh* mesh = nullptr;
    log.call("sgs_mesh_upload", sgs_mesh_upload(ctx, 8, in.verts.data(), 12, in.tris.data(), 0, &mesh));
    log.call("sgs_mesh_set_labels", sgs_mesh_set_labels(ctx, mesh, in.labels.data(), 0), !mesh);
    std::vector<float> depth((size_t)W0 * H0, -1.0f), depth2((size_t)2 * W0 * H0, -1.0f);
    std::vector<int32_t> ids((size_t)W0 * H0, -7), ids2((size_t)2 * W0 * H0, -7);
    const sgs_camera mcams[2] = {make_camera(W0, H0, 0.0f), make_camera(W0, H0, 0.4f)};
    log.call("sgs_render_mesh_depth", sgs_render_mesh_depth(ctx, mesh, &mcams[0], &cfg, 0, -1, depth.data(), &st, nullptr), !mesh);
    log.keep(depth);
    log.call("sgs_render_mesh_ids", sgs_render_mesh_ids(ctx, mesh, &mcams[0], &cfg, 0, -1, depth.data(), ids.data(), &st, nullptr), !mesh);
    log.keep(depth); log.keep(ids);
    log.call("sgs_render_mesh_ids_batch of 2", sgs_render_mesh_ids_batch(ctx, mesh, mcams, 2, &cfg, depth2.data(), ids2.data(), nullptr, nullptr), !mesh);
    log.keep(depth2); log.keep(ids2);
    log.call("sgs_mesh_set_record_capacity (1)", sgs_mesh_set_record_capacity(ctx, 1));
    sgs_stats mst[2];
    mst[0].retries = -1;
    log.call("sgs_render_mesh_depth_batch of 2, rendered again", sgs_render_mesh_depth_batch(ctx, mesh, mcams, 2, &cfg, depth2.data(), mst, nullptr), !mesh);
    log.retried.push_back(mst[0].retries);
    log.keep(depth2);

    // ---- what is made of the frames
    if (rgb0.empty()) rgb0.assign((size_t)W0 * H0 * 3, 0.25f);          // (its frame was refused)
    for (int n : {1, 3}) {
        sgs_jpeg_params p;
        sgs_jpeg_params_default(&p);
        const int64_t cap = n * sgs_jpeg_bound(W0, H0, &p);
        std::vector<uint8_t> files((size_t)cap, 0);
        std::vector<int64_t> offs((size_t)n, -1), sizes((size_t)n, -1);
        log.call("sgs_encode_jpeg", sgs_encode_jpeg(ctx, n == 1 ? rgb0.data() : batch.data(), W0, H0, n, (int64_t)W0 * H0 * 3, &p, files.data(), cap,
                                                    offs.data(), sizes.data(), nullptr));
        log.call("sgs_jpeg_status", sgs_jpeg_status(ctx, nullptr));
        log.keep(files); log.keep(offs); log.keep(sizes);
    }
    for (int format : {SGS_PNG_RGB8, SGS_PNG_DEPTH16}) {
        sgs_png_params p;
        sgs_png_params_default(&p);
        p.format = format;
        const int n = 2;
        const int64_t cap = n * sgs_png_bound(W0, H0, &p);
        std::vector<uint8_t> files((size_t)cap, 0);
        std::vector<int64_t> offs((size_t)n, -1), sizes((size_t)n, -1);
        log.call("sgs_encode_png", sgs_encode_png(ctx, format == SGS_PNG_RGB8 ? batch.data() : depth2.data(), W0, H0, n,
                                                  (int64_t)W0 * H0 * (format == SGS_PNG_RGB8 ? 3 : 1), &p, files.data(), cap, offs.data(), sizes.data(), nullptr));
        log.call("sgs_png_status", sgs_png_status(ctx, nullptr));
        log.keep(files); log.keep(offs); log.keep(sizes);
    }
    for (int filter : {SGS_RESIZE_BICUBIC, SGS_RESIZE_LINEAR}) {
        sgs_resize_params p;
        sgs_resize_params_default(&p);
        p.filter = filter; p.dst_width = 20; p.dst_height = 12;
        std::vector<float> dst((size_t)20 * 12 * 3, -1.0f);
        log.call("sgs_resize", sgs_resize(ctx, rgb0.data(), W0, H0, 1, 0, &p, dst.data(), 0, nullptr));
        log.keep(dst);
    }
    {
        std::vector<sgs_object_row> rows(2 * 6);
        memset(rows.data(), 0x5a, rows.size() * sizeof(sgs_object_row));
        std::vector<uint32_t> counts(2 * 2, 0x5a5a5a5au);
        log.call("sgs_object_table", sgs_object_table(ctx, ids2.data(), depth2.data(), 2, H0, W0, (int64_t)W0 * H0, 6, rows.data(), counts.data(), nullptr));
        log.keep(rows); log.keep(counts);
    }

    log.call("sgs_mesh_free", sgs_mesh_free(ctx, mesh));
    log.call("sgs_scene_free", sgs_scene_free(ctx, packed));
    log.call("sgs_scene_free", sgs_scene_free(ctx, large));
    log.call("sgs_scene_free", sgs_scene_free(ctx, small_));
}

sgs_ctx* create() {
    sgs_ctx* ctx = nullptr;
    if (sgs_create(0, SGS_BACKEND_HIP, &ctx) != SGS_OK) { fprintf(stderr, "walk: sgs_create: %s\n", sgs_last_error(nullptr)); exit(2); }
    // (a small record capacity from the start: whatever the script's own first call meets, no lane allocates the default 16 Mi records)
    if (sgs_set_record_capacity(ctx, 1 << 15) != SGS_OK) { fprintf(stderr, "walk: sgs_set_record_capacity: %s\n", sgs_last_error(ctx)); exit(2); }
    return ctx;
}

}  // namespace

int main(int argc, char** argv) {
    const Inputs in;
    Log ref;
    ref.verbose = getenv("WALK_VERBOSE") != nullptr;
    sgs_ctx* ctx = create();
    const long long before = hipemu::alloc_count;
    script(ctx, in, ref);
    const long long N = hipemu::alloc_count - before;
    sgs_destroy(ctx);
    for (size_t i = 0; i < ref.rc.size(); ++i)
        if (ref.rc[i] < 0) { fprintf(stderr, "walk: call %zu of the unfailed script returned %lld\n", i, ref.rc[i]); return 2; }
    for (int r : ref.retried)
        if (r < 1) { fprintf(stderr, "walk: a frame that was to overflow its record buffer did not (retries = %d)\n", r); return 2; }
    const long long k0 = argc > 1 ? atoll(argv[1]) : 0, k1 = argc > 2 ? atoll(argv[2]) : N;
    fprintf(stderr, "walk: %zu calls, %zu outputs, %lld allocations; k in [%lld, %lld)\n", ref.rc.size(), ref.out.size(), N, k0, k1);
    int failures = 0;
    if (k0 == 0) {      // sgs_create's own allocations, before the script's
        long long n_create = hipemu::alloc_count;
        sgs_ctx* c = nullptr;
        if (sgs_create(0, SGS_BACKEND_HIP, &c) != SGS_OK) return 2;
        n_create = hipemu::alloc_count - n_create;
        sgs_destroy(c);
        for (long long k = 0; k < n_create; ++k) {
            c = nullptr;
            hipemu::alloc_fail_in = k;
            const int rc = sgs_create(0, SGS_BACKEND_HIP, &c);
            const bool fired = hipemu::alloc_fail_in < 0;
            hipemu::alloc_fail_in = -1;
            if (!fired || rc == SGS_OK || c) { fprintf(stderr, "walk: sgs_create with its allocation %lld refused returned %d\n", k, rc); ++failures; sgs_destroy(c); }
        }
        fprintf(stderr, "walk: sgs_create: %lld allocations refused in turn\n", n_create);
    }
    for (long long k = k0; k < k1 && k < N; ++k) {
        fprintf(stderr, "walk: k = %lld\n", k);
        ctx = create();
        Log failed, again;
        hipemu::alloc_fail_in = k;
        script(ctx, in, failed);
        const bool fired = hipemu::alloc_fail_in < 0;
        hipemu::alloc_fail_in = -1;
        script(ctx, in, again);
        sgs_destroy(ctx);
        int wrong = failed.bad;
        if (!fired) { fprintf(stderr, "walk: k = %lld: the script made fewer allocations than the unfailed one\n", k); ++wrong; }
        if (fired && !failed.refused) { fprintf(stderr, "walk: k = %lld: an allocation was refused and no call said so\n", k); ++wrong; }
        if (again.rc != ref.rc) {
            for (size_t i = 0; i < ref.rc.size(); ++i)
                if (again.rc[i] != ref.rc[i]) fprintf(stderr, "walk: k = %lld: call %zu returns %lld after the failure, %lld without\n", k, i, again.rc[i], ref.rc[i]);
            ++wrong;
        }
        for (size_t i = 0; i < ref.out.size(); ++i)
            if (again.out[i] != ref.out[i]) { fprintf(stderr, "walk: k = %lld: output %zu differs after the failure\n", k, i); ++wrong; }
        if (wrong) { fprintf(stderr, "walk: k = %lld FAILED\n", k); ++failures; }
    }
    fprintf(stderr, "walk: %d of %lld failure points wrong\n", failures, std::min(k1, N) - k0);
    return failures ? 1 : 0;
}
