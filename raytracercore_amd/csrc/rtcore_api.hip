// rtcore_api.hip -- the C ABI (include/rtcore.h): the scene's life cycle and the render entry
// points.  Scene upload and launches: scene_upload.hip; the multi-GPU frame: api_frame.hip; the
// host-only and experiment entry points: api_debug.hip.
//
// Replaces the body of the reference's render worker loop (Raytracer.Render,
// Raytracer.cs:294-330) behind FullRaytracer's GetWorkingTile / OnTileFinished contract
// (FullRaytracer.cs:210-229); see INTEGRATION.md for the C# P/Invoke side.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>

#include "rt_scene.h"

namespace rtc {
static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
} // namespace rtc

extern "C" {

int rt_set_jit(int32_t on)
{
    if (on != 0 && on != 1) {
        set_error("rt_set_jit: on must be 0 or 1");
        return RT_ERR_ARG;
    }
    jit_set_enabled(on == 1);
    return RT_OK;
}

int rt_scene_get_jit_error(const rt_scene* s, char* buf, int32_t cap)
{
    if (!s || !buf || cap <= 0) {
        set_error("rt_scene_get_jit_error: bad argument");
        return RT_ERR_ARG;
    }
    const std::string& e = s->jit.error;
    const size_t n = std::min((size_t)cap - 1, e.size());
    memcpy(buf, e.data(), n);
    buf[n] = '\0';
    return (int)e.size();
}

int rt_scene_get_build_stats(const rt_scene* s, double* out, int32_t n)
{
    if (!s || !out || n < 0) {
        set_error("rt_scene_get_build_stats: bad argument");
        return RT_ERR_ARG;
    }
    const auto& L = s->layout;
    const double v[RT_BUILD_STATS_COUNT] = {s->ms_prepare, s->ms_bvh, s->ms_upload, (double)s->bvh.gpu_ms,
                                           (double)s->bvh.rounds, (double)s->bvh.n_nodes4, (double)s->bvh.stack4,
                                           (double)L.rects, (double)L.boxes, (double)L.frames, (double)L.frame_boxes,
                                           (double)L.frame_rects, (double)L.tris, (double)L.sphs,
                                           (double)s->dev.n_hot4, (double)s->jit.status, s->jit.compile_ms,
                                           s->jit.from_cache ? 1.0 : 0.0, (double)s->group_max,
                                           (double)s->bvh.leaves4, (double)s->bvh.compact4,
                                           (double)std::count(s->bvh_outer.begin(), s->bvh_outer.end(), 1)};
    for (int i = 0; i < n && i < RT_BUILD_STATS_COUNT; i++) out[i] = v[i];
    return RT_OK;
}

int rt_abi_version(void) { return RTCORE_ABI_VERSION; }

int rt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_last_error(char* buf, int32_t cap)
{
    if (buf && cap > 0) {
        std::strncpy(buf, g_error.c_str(), (size_t)cap - 1);
        buf[cap - 1] = 0;
    }
    return (int)g_error.size();
}

int rt_scene_create(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims, int32_t device,
                    rt_scene** out_scene)
{
    if (!params || !out_scene || n_prims < 0 || (n_prims > 0 && !prims)) {
        set_error("rt_scene_create: bad argument");
        return RT_ERR_ARG;
    }
    *out_scene = nullptr;
    if (params->width <= 0 || params->height <= 0) {
        set_error("rt_scene_create: width and height must be positive");
        return RT_ERR_ARG;
    }
    if (params->width > 65535 || params->height > 65535) { // the BVH kernels pack a pixel's x, y in 16 bits each
        set_error("rt_scene_create: width and height must be at most 65535");
        return RT_ERR_ARG;
    }
    for (int i = 0; i < n_prims; i++)
        if (prims[i].kind < 0 || prims[i].kind > 2) {
            set_error("rt_scene_create: unknown primitive kind at index " + std::to_string(i));
            return RT_ERR_ARG;
        }
    int ndev = rt_device_count();
    if (ndev <= 0) {
        set_error("rt_scene_create: no HIP device");
        return RT_ERR_NODEVICE;
    }
    if (device < 0 || device >= ndev) {
        set_error("rt_scene_create: device index out of range");
        return RT_ERR_ARG;
    }
    std::unique_ptr<rt_scene> s(new rt_scene());
    s->device = device;
    s->params = *params;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    s->n_cu = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    // the launch sets' streams, created one after the other: the runtime deals hardware queues to streams
    // in the order they are created, and two streams on one queue run in submission order
    for (rt_scene::LaunchSet& l : s->sets) {
        HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&l.path_done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&l.fold_done, hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&s->shared_ev, hipEventDisableTiming));
    for (int i = 0; i < rt_scene::kTimeSlots; i++) {
        HIP_TRY(hipEventCreate(&s->t_start[i]));
        HIP_TRY(hipEventCreate(&s->t_end[i]));
    }
    HIP_TRY(hipEventCreateWithFlags(&s->done_ev, hipEventDisableTiming));
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::duration d) { return std::chrono::duration<double, std::milli>(d).count(); };
    const auto t0 = clk::now();
    s->host = prepare_prims(prims, n_prims);
    const auto t1 = clk::now();
    int rc = build_bvhs(s.get());
    if (rc != RT_OK) return rc;
    const auto t2 = clk::now();
    rc = upload_scene(s.get());
    if (rc != RT_OK) return rc;
    s->ms_prepare = ms(t1 - t0);
    s->ms_bvh = ms(t2 - t1);
    s->ms_upload = ms(clk::now() - t2);
    rc = resolve_traversal(s.get());
    if (rc != RT_OK) return rc;
    HIP_TRY(s->rays.reserve(1));
    HIP_TRY(s->set_rays.reserve(2));
    HIP_TRY(hipMemset(s->set_rays.p, 0, 2 * sizeof(unsigned long long)));
    *out_scene = s.release();
    return RT_OK;
}

int rt_scene_set_camera(rt_scene* s, const rt_camera* cam)
{
    if (!s || !cam || (cam->kind != RT_CAMERA_FRUSTUM && cam->kind != RT_CAMERA_ORTHO)) {
        set_error("rt_scene_set_camera: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    camera_init(*cam, s->params.width, s->params.height, s->camd, s->camf);
    // launches of the previous camera may still be in flight on any stream
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(s->camf_d.reserve(1));
    HIP_TRY(hipMemcpy(s->camf_d.p, &s->camf, sizeof(CameraF), hipMemcpyHostToDevice));
    // The grouped order's groups nearest to the camera first: camera rays find their closest hit
    // early and skip the primitives of groups behind it (each group owns its own ranges, so only
    // the GroupRec order changes).  Deterministic for a given scene and camera.
    if (s->groups_gr_host.size() > 1 && !getenv("RTCORE_NO_GROUP_SORT")) {
        const std::vector<GroupRec> g = groups_nearest_first(s->groups_gr_host, s->camd);
        HIP_TRY(hipMemcpy(s->grouped_d.groups.p, g.data(), g.size() * sizeof(GroupRec), hipMemcpyHostToDevice));
        s->grouped_h.groups = g; // the order the scene-specialised grouped kernel is built with
    }
    s->has_camera = true;
    s->cam_gen++; // the block cull's records are per camera
    s->jit_gen++; // the scene-specialised kernel carries the camera (and the group order)
    const int rc = calibrate_grouping(s);
    if (rc == RT_OK) (void)prepare_jit(s); // build the scene-specialised kernel now, not in a launch
    return rc;
}

int rt_scene_set_traversal(rt_scene* s, int32_t traversal)
{
    if (!s || traversal < RT_TRAVERSAL_AUTO || traversal > RT_TRAVERSAL_GROUPED) {
        set_error("rt_scene_set_traversal: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    const int before = s->traversal;
    s->traversal = traversal;
    const int rc = (traversal == RT_TRAVERSAL_AUTO && s->has_camera) ? calibrate_grouping(s) : resolve_traversal(s);
    if (rc != RT_OK) {
        s->traversal = before; // a refused mode leaves the scene as it was
        return rc;
    }
    if (s->has_camera) (void)prepare_jit(s);
    return rc;
}

int rt_scene_get_info(const rt_scene* s, rt_scene_info* info)
{
    if (!s || !info) {
        set_error("rt_scene_get_info: bad argument");
        return RT_ERR_ARG;
    }
    std::memset(info, 0, sizeof *info);
    info->n_prims = (int32_t)s->host.size();
    info->ref_bvh_nodes = (int32_t)s->ref.nodes.size();
    info->ref_bvh_depth = s->ref.depth;
    info->sah_bvh_nodes = s->bvh.n_nodes2;
    info->sah_bvh_depth = s->bvh.depth2;
    info->bvh_builder = s->bvh.builder;
    info->traversal = s->resolved;
    info->device = s->device;
    info->device_bytes = s->device_bytes;
    return RT_OK;
}

void rt_scene_destroy(rt_scene* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    for (rt_scene::LaunchSet& l : s->sets)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    delete s;
}

int rt_render_device(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp, uint64_t seed,
                     uint64_t sample_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                     unsigned long long* d_rays, void* stream)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    if (spp <= 0 || !d_sum || !d_samples || !d_misses || !d_rays) {
        set_error("rt_render_device: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params(s, x0, y0, w, h, spp, seed, sample_base);
    rc = run_path(s, p, d_rays, st, true, true);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate(p, d_sum, d_samples, d_misses, st, 0, s->open_set >= 0 ? s->set_rays.p + s->open_set : nullptr,
                              d_rays));
    return end_op(s, st);
}

int rt_kernel_times(rt_scene* s, int32_t n, float* ms)
{
    if (!s || !ms || n < 1 || n > rt_scene::kTimeRing || (uint64_t)n > s->launches) {
        set_error("rt_kernel_times: bad argument (n must be 1.." + std::to_string(rt_scene::kTimeRing) +
                  " and at most the launches so far)");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    // The time a launch had to itself: t_end[k] - max(t_start[k], t_end[k - 1]).  An overlapped launch's
    // start event fires while the launch before it still runs, and the raw pair would count that time
    // twice; for a serial launch the predecessor ended before the start, and this is the raw pair.
    for (int i = 0; i < n; i++) { // oldest first
        const uint64_t k = s->launches - (uint64_t)n + (uint64_t)i;
        const int slot = (int)(k % rt_scene::kTimeSlots);
        HIP_TRY(hipEventSynchronize(s->t_end[slot]));
        HIP_TRY(hipEventElapsedTime(ms + i, s->t_start[slot], s->t_end[slot]));
        if (k > 0) {
            const int prev = (int)((k - 1) % rt_scene::kTimeSlots);
            float since = 0.0f;
            HIP_TRY(hipEventSynchronize(s->t_end[prev]));
            HIP_TRY(hipEventElapsedTime(&since, s->t_end[prev], s->t_end[slot]));
            if (since > 0.0f && since < ms[i]) ms[i] = since;
        }
    }
    return RT_OK;
}

// rt_kernel_times' entries as the raw event pairs t_end[k] - t_start[k] (tests: what rt_kernel_times makes of them).
int rt_debug_kernel_times_raw(rt_scene* s, int32_t n, float* ms)
{
    if (!s || !ms || n < 1 || n > rt_scene::kTimeRing || (uint64_t)n > s->launches) {
        set_error("rt_debug_kernel_times_raw: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    for (int i = 0; i < n; i++) {
        const int slot = (int)((s->launches - (uint64_t)n + (uint64_t)i) % rt_scene::kTimeSlots);
        HIP_TRY(hipEventSynchronize(s->t_end[slot]));
        HIP_TRY(hipEventElapsedTime(ms + i, s->t_start[slot], s->t_end[slot]));
    }
    return RT_OK;
}

int rt_last_kernel_ms(rt_scene* s, float* ms)
{
    if (!s || !ms) {
        set_error("rt_last_kernel_ms: bad argument");
        return RT_ERR_ARG;
    }
    if (s->launches == 0) {
        set_error("rt_last_kernel_ms: no path kernel launched on this scene yet");
        return RT_ERR_ARG;
    }
    return rt_kernel_times(s, 1, ms);
}

int rt_scene_set_stats(rt_scene* s, int32_t enable)
{
    if (!s) {
        set_error("rt_scene_set_stats: null scene");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    if (enable) {
        HIP_TRY(s->stats_buf.reserve(RT_STATS_COUNT));
        HIP_TRY(hipMemset(s->stats_buf.p, 0, RT_STATS_COUNT * sizeof(unsigned long long)));
        s->stats_blocks_per_cu = path_blocks_per_cu(s->variant, path_dyn_lds(s->dev, s->variant), true, s->dev.n_vn > 0);
    }
    s->stats_on = enable != 0;
    return RT_OK;
}

int rt_scene_get_stats(rt_scene* s, uint64_t* out, int32_t n)
{
    if (!s || !out || n < 0) {
        set_error("rt_scene_get_stats: bad argument");
        return RT_ERR_ARG;
    }
    if (!s->stats_buf.p) {
        set_error("rt_scene_get_stats: statistics were never enabled");
        return RT_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[RT_STATS_COUNT];
    HIP_TRY(hipMemcpy(v, s->stats_buf.p, sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(s->stats_buf.p, 0, sizeof v));
    for (int k = 0; k < n && k < RT_STATS_COUNT; k++) out[k] = v[k];
    return RT_OK;
}

int rt_render_tile(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp, uint64_t seed,
                   uint64_t sample_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    if (spp < 0 || !sum_rgb || !samples || !misses) {
        set_error("rt_render_tile: bad argument");
        return RT_ERR_ARG;
    }
    if (spp == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    // A previous call that failed between its first queued copy and its consume step may have left
    // band copies in flight on copy_stream, reading colors into stage: both are about to be
    // reserved (maybe reallocated), so wait for them first (normally the stream is already idle).
    if (s->copy_stream) HIP_TRY(hipStreamSynchronize(s->copy_stream));
    const size_t npix = (size_t)w * h;
    HIP_TRY(s->sum.reserve(3 * npix));
    HIP_TRY(s->samples.reserve(npix));
    HIP_TRY(s->misses.reserve(npix));
    HIP_TRY(s->colors.reserve(4 * npix)); // the caller's layout: one 32-B TileRec per pixel, x*h + y
    HIP_TRY(s->stage.reserve(npix * sizeof(TileRec)));
    HIP_TRY(s->rays_h.reserve(1));
    HIP_TRY(hipMemsetAsync(s->sum.p, 0, 3 * npix * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->samples.p, 0, npix * sizeof(uint32_t), s->stream));
    HIP_TRY(hipMemsetAsync(s->misses.p, 0, npix * sizeof(uint32_t), s->stream));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
    TileRec* d_rec = reinterpret_cast<TileRec*>(s->colors.p);
    // A large call renders in column bands, each a launch of its own whose records are copied (on
    // copy_stream) and added into the caller's arrays (the band's columns are one contiguous range
    // of x*h + y) while the next band renders: only the last band's copy and add are not hidden
    // behind the kernel.  Every band launch takes the whole tile's chunks per pixel, so the sums are
    // those of one launch bit for bit.  bounce.txt 1080p, ms per call into the caller's arrays
    // with 1 / 2 / 4 bands (tools/host_path_timing.py, profiles/r04/host_path_bands.log): 16 spp
    // 4.17 / 3.89 / 3.54, 64 spp 8.13 / 7.88 / 7.21, 256 spp 22.05 / 20.95 / 20.86; after the
    // round's kernel gains (profiles/r04/host_path_timing.log, 1 / 4 bands) 16 spp 4.33 / 4.00, 64 spp
    // 7.99 / 7.49, 256 spp 19.86 / 20.04: a long call gains less from the overlap than its band
    // launches' tails cost, so from 2.5e8 samples per call it is one launch again.
    // RTCORE_TILE_BANDS overrides the count (1 = one launch).
    const double work = (double)npix * spp;
    int nb = work >= 2.5e8 ? 1 : work >= 1.6e7 ? 4 : work >= 4e6 ? 2 : 1;
    if (const char* e = getenv("RTCORE_TILE_BANDS")) nb = std::max(1, std::min(4, atoi(e)));
    nb = std::max(1, std::min(nb, w / 64));
    if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    const int per_band_chunks = nb == 1 ? (int)std::max<size_t>(1, std::min<size_t>(rt_scene::kCopyChunks,
                                                                                  (npix * sizeof(TileRec)) >> 20))
                                        : rt_scene::kCopyChunks / nb;
    CopyPlan plan;
    for (int k = 0; k < nb; k++) {
        const int a = nb == 1 ? 0 : (int)((int64_t)w * k / nb) & ~7, b = k + 1 == nb ? w : (int)((int64_t)w * (k + 1) / nb) & ~7;
        const int wb = b - a;
        const size_t off = (size_t)a * h;
        PathParams p = make_params(s, x0 + a, y0, wb, h, spp, seed, sample_base, (double)npix);
        rc = run_path(s, p, s->rays.p, s->stream);
        if (rc != RT_OK) return rc;
        HIP_TRY(launch_accumulate(p, s->sum.p + 3 * off, s->samples.p + off, s->misses.p + off, s->stream));
        HIP_TRY(launch_tile_host_layout(wb, h, s->sum.p + 3 * off, s->samples.p + off, s->misses.p + off, d_rec + off,
                                        s->stream));
        if (!s->band_ev[k]) HIP_TRY(hipEventCreateWithFlags(&s->band_ev[k], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->band_ev[k], s->stream));
        HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->band_ev[k], 0));
        if (k + 1 == nb) // (before the last chunks, so it has landed when they have)
            HIP_TRY(hipMemcpyAsync(s->rays_h.p, s->rays.p, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   s->copy_stream));
        rc = queue_copy(s, plan, d_rec, off, off + (size_t)wb * h, sizeof(TileRec), per_band_chunks, s->copy_stream);
        if (rc != RT_OK) return rc;
    }
    rc = end_op(s, s->stream);
    if (rc != RT_OK) return rc;
    rc = consume_copies(s, plan, [&](const unsigned char* st, size_t a, size_t b) {
        const TileRec* r = reinterpret_cast<const TileRec*>(st);
        for (size_t o = a; o < b; o++) {
            sum_rgb[o].r += r[o].r;
            sum_rgb[o].g += r[o].g;
            sum_rgb[o].b += r[o].b;
            samples[o] += r[o].samples;
            misses[o] += r[o].misses;
        }
    });
    if (rc != RT_OK) return rc;
    if (rays_out) *rays_out += s->rays_h.p[0]; // copied before the last band's chunks, on the copy stream
    return RT_OK;
}

int rt_render_tile_1spp(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, uint64_t seed,
                        uint64_t sample_index, rt_color* out)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    if (!out) {
        set_error("rt_render_tile_1spp: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t npix = (size_t)w * h;
    HIP_TRY(s->colors32.reserve(3 * npix));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
    PathParams p = make_params(s, x0, y0, w, h, 1, seed, sample_index);
    rc = run_path(s, p, s->rays.p, s->stream);
    if (rc != RT_OK) return rc;
    // the pass as fp32 in the caller's order (the kernel's sample values are fp32: widened exactly
    // on the host), 12 B per pixel over PCIe instead of 24, in chunks widened as they land
    HIP_TRY(launch_colors_1spp(p, s->colors32.p, s->stream));
    rc = end_op(s, s->stream);
    if (rc != RT_OK) return rc;
    return copy_consume(s, s->colors32.p, npix, 3 * sizeof(float), [&](const unsigned char* st, size_t a, size_t b) {
        const float* f = reinterpret_cast<const float*>(st);
        for (size_t o = a; o < b; o++) out[o] = rt_color{(double)f[3 * o], (double)f[3 * o + 1], (double)f[3 * o + 2]};
    });
}

// Raytracer.GetDebugTrace for the library's own samples: the instrumented instance of the scene's
// path kernel (the record code is compiled into those instances only) over the tile, launched as a
// render of the tile is (make_params: the same items), then the records in the caller's order.
int rt_trace_paths(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp, uint64_t seed,
                   uint64_t sample_base, rt_debug_ray* rays_out, int32_t* n_rays_out, rt_color* colors_out)
{
    static_assert(sizeof(rt_debug_ray) == kRecRows * sizeof(float4), "rt_debug_ray is kRecRows float4 rows");
    if (!rays_out || spp <= 0 || w <= 0 || h <= 0) {
        set_error("rt_trace_paths: bad argument (null rays_out, or spp, w or h <= 0)");
        return RT_ERR_ARG;
    }
    // (a path has at least one record, so this holds whatever the scene's recursion is)
    if ((uint64_t)w * (uint64_t)h * (uint64_t)spp > (uint64_t)RT_TRACE_MAX_RECORDS) {
        set_error("rt_trace_paths: more than RT_TRACE_MAX_RECORDS records; trace fewer pixels or samples");
        return RT_ERR_ARG;
    }
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    const size_t n_samples = (size_t)w * h * spp;
    const size_t per = (size_t)s->params.recursion + 1; // records of a sample (Raytracer.cs:257)
    const size_t n_rec = n_samples * per;
    if (s->params.recursion < 0 || n_rec > (size_t)RT_TRACE_MAX_RECORDS) {
        set_error("rt_trace_paths: more than RT_TRACE_MAX_RECORDS records; trace fewer pixels or samples");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t rec_rows = n_rec * kRecRows;
    HIP_TRY(s->trace_rays.reserve(rec_rows));
    HIP_TRY(s->trace_samples.reserve(n_samples));
    HIP_TRY(s->trace_out.reserve(rec_rows + n_samples));
    HIP_TRY(s->trace_stats.reserve(RT_STATS_COUNT));
    HIP_TRY(hipMemsetAsync(s->trace_rays.p, 0, rec_rows * sizeof(float4), s->stream));
    HIP_TRY(hipMemsetAsync(s->trace_samples.p, 0, n_samples * sizeof(float4), s->stream));
    HIP_TRY(hipMemsetAsync(s->trace_stats.p, 0, RT_STATS_COUNT * sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
    PathParams p = make_params(s, x0, y0, w, h, spp, seed, sample_base);
    p.rec_rays = s->trace_rays.p;
    p.rec_samples = s->trace_samples.p;
    p.rec_max = (unsigned)n_rec;
    // the instrumented instance for this one launch, as calibrate_grouping borrows it
    const bool was_on = s->stats_on;
    const int was_blocks = s->stats_blocks_per_cu;
    s->stats_on = s->tracing = true;
    s->stats_blocks_per_cu = path_blocks_per_cu(s->variant, path_dyn_lds(s->dev, s->variant), true, s->dev.n_vn > 0);
    rc = run_path(s, p, s->rays.p, s->stream, false); // not one of rt_kernel_times' launches
    s->stats_on = was_on;
    s->tracing = false;
    s->stats_blocks_per_cu = was_blocks;
    if (rc != RT_OK) return rc;
    float4* d_rays = s->trace_out.p;
    float4* d_samples = s->trace_out.p + rec_rows;
    HIP_TRY(launch_trace_host_layout(w, h, spp, s->params.recursion, s->trace_rays.p, s->trace_samples.p, d_rays, d_samples,
                                     s->stream));
    rc = end_op(s, s->stream);
    if (rc != RT_OK) return rc;
    rc = copy_consume(s, d_rays, n_rec, sizeof(rt_debug_ray), [&](const unsigned char* st, size_t a, size_t b) {
        std::memcpy(rays_out + a, st + a * sizeof(rt_debug_ray), (b - a) * sizeof(rt_debug_ray));
    });
    if (rc != RT_OK) return rc;
    // a sample's row: its fp32 colour (widened exactly, as rt_render_tile_1spp's) and its record count
    return copy_consume(s, d_samples, n_samples, sizeof(float4), [&](const unsigned char* st, size_t a, size_t b) {
        const float* f = reinterpret_cast<const float*>(st);
        for (size_t o = a; o < b; o++) {
            if (colors_out) colors_out[o] = rt_color{(double)f[4 * o], (double)f[4 * o + 1], (double)f[4 * o + 2]};
            if (n_rays_out) std::memcpy(&n_rays_out[o], &f[4 * o + 3], sizeof(int32_t));
        }
    });
}

} // extern "C"

namespace {

// The exact fp64 debug passes (DebugRaycaster.cs:170-212): mode 0 primary hit IDs, mode 1
// reference-BVH node counts.  Device output is row-major over the tile.
int debug_pass_device(rt_scene* s, int mode, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* d_out,
                      hipStream_t stream, const char* name)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    if (!d_out) {
        set_error(std::string(name) + ": bad argument");
        return RT_ERR_ARG;
    }
    rc = ensure_ref_bvh(s);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(launch_primary_ids(s->dev, s->camd, x0, y0, w, h, mode, d_out, stream));
    return RT_OK;
}

// The same into a host buffer in the DoubleColor[w, h]-style x*h + y order.
int debug_pass_host(rt_scene* s, int mode, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* out, const char* name)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    if (!out) {
        set_error(std::string(name) + ": bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t npix = (size_t)w * h;
    HIP_TRY(s->ids.reserve(npix));
    rc = debug_pass_device(s, mode, x0, y0, w, h, s->ids.p, s->stream, name);
    if (rc != RT_OK) return rc;
    std::vector<int32_t> tmp(npix);
    HIP_TRY(hipMemcpyAsync(tmp.data(), s->ids.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::atomic<bool> overflow{false};
    parallel_ranges((size_t)w, 64, [&](size_t xa, size_t xb) { // column ranges: disjoint output spans
        bool of = false;
        for (int y = 0; y < h; y++)
            for (size_t x = xa; x < xb; x++) {
                const int32_t v = tmp[(size_t)y * w + x];
                of |= v == -2;
                out[x * h + y] = v;
            }
        if (of) overflow = true;
    });
    if (overflow) {
        set_error(std::string(name) + ": the reference BVH is deeper than the exact kernel's traversal stack");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_primary_ids_device(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* d_ids, void* stream)
{
    return debug_pass_device(s, 0, x0, y0, w, h, d_ids, static_cast<hipStream_t>(stream), "rt_primary_ids_device");
}

int rt_primary_ids(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* ids_out)
{
    return debug_pass_host(s, 0, x0, y0, w, h, ids_out, "rt_primary_ids");
}

int rt_bvh_counts(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* counts_out)
{
    return debug_pass_host(s, 1, x0, y0, w, h, counts_out, "rt_bvh_counts");
}

} // extern "C"

extern "C" {

int rt_tonemap_device(const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses, int32_t w, int32_t h,
                      rt_color background, double background_alpha, double exposure, int32_t* d_argb, void* stream)
{
    if (!d_sum || !d_samples || !d_misses || !d_argb || w <= 0 || h <= 0) {
        set_error("rt_tonemap_device: bad argument");
        return RT_ERR_ARG;
    }
    HIP_TRY(launch_tonemap(w, h, d_sum, d_samples, d_misses, background, background_alpha, exposure, d_argb,
                           static_cast<hipStream_t>(stream)));
    return RT_OK;
}

int32_t rt_sample_output(rt_color sum, uint32_t n_samples, uint32_t n_misses, rt_color back, double back_alpha,
                         double exposure)
{
    // SampleSet.GetOutput / GetColorCode (SampleSet.cs:50-113) with Util.Clamp's SSE form
    auto clamp01 = [](double v) {
        v = v > 0.0 ? v : 0.0;
        return v < 1.0 ? v : 1.0;
    };
    auto code = [&](double r, double g, double b, double a) {
        return (int32_t)(((uint32_t)(int32_t)(clamp01(a) * 255) << 24) | ((uint32_t)(int32_t)(clamp01(r) * 255) << 16) |
                         ((uint32_t)(int32_t)(clamp01(g) * 255) << 8) | (uint32_t)(int32_t)(clamp01(b) * 255));
    };
    if (n_samples == 0) return code(back.r * exposure, back.g * exposure, back.b * exposure, back_alpha);
    double total = (double)n_samples + (double)n_misses;
    double mult = exposure / n_samples;
    double r = sum.r * mult, g = sum.g * mult, b = sum.b * mult, a = 1;
    double bam = n_misses / total, bk = bam * back_alpha;
    r += (back.r - r) * bk;
    g += (back.g - g) * bk;
    b += (back.b - b) * bk;
    a += (back_alpha - a) * bam;
    const double gamma = 1 / 2.2;
    return code(pow(r, gamma), pow(g, gamma), pow(b, gamma), a);
}

} // extern "C"
