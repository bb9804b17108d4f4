// api_render_pixels.hip -- the C ABI's list renders (include/rtcore.h, "adaptive sampling"): the
// camera's own samples of a list of frame pixels, by the PIXELS instances of the path kernels
// (kernels_path.hip, refill), folded into whole-frame accumulators with the moments of the error estimate.
#include <cstring>

#include "rt_scene.h"

namespace {

constexpr int64_t kPixelsChunk = 1 << 19; // entries of one chunk of rt_render_pixels (rt_render_rays' size and variable)

// run_items for the PIXELS instance over the n entries at d_pixels: the camera and the pixel-key table in the
// rays' place, no block cull.
int run_pixels(rt_scene* s, PathParams& p, const uint32_t* d_pixels, unsigned long long* d_count, hipStream_t stream)
{
    p.pixel_list = d_pixels;
    p.cull = nullptr;
    return run_items(s, ITEMS_PIXELS, "pixels", p, d_count, stream);
}

// Argument and state checks shared by both entry points; RT_OK with *empty set for n == 0.
int check_render_pixels(rt_scene* s, const void* pixels, int64_t n, int32_t spp, const void* sum, const void* samples,
                        const void* misses, const void* q, const void* batches, const char* name, bool* empty)
{
    *empty = false;
    const char* bad = !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && (q != nullptr) != (batches != nullptr)) bad = "q and batches go together";
    if (!bad && n == 0) { // (as rt_render_rays: an empty list may come with null arrays)
        *empty = true;
        return RT_OK;
    }
    if (!bad && (!pixels || !sum || !samples || !misses)) bad = "null pointer";
    if (!bad && (uint64_t)s->params.width * (uint64_t)s->params.height >= (1ull << 32)) bad = "a frame of 2^32 pixels or more";
    if (!bad && s->params.height > (1 << 20)) bad = "a frame of more than 2^20 rows"; // (list_pixel's division)
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    if (!s->has_camera) {
        set_error(std::string(name) + ": no camera set (rt_scene_set_camera)");
        return RT_ERR_STATE;
    }
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": runs in the traversal modes BRUTE, GROUPED and BVH; this scene is in BVH2 mode "
                                      "(rt_scene_set_traversal), use RT_TRAVERSAL_BVH");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

} // namespace

namespace rtc {

// The host entry's list check: every entry inside the frame and none named twice, by a bitmap of the
// frame (npix bits).  Returns null, or what is wrong and the first offending entry's index.
const char* check_pixel_list(const uint32_t* pixels, int64_t n, uint64_t npix, int64_t* at)
{
    std::vector<uint64_t> seen((size_t)((npix + 63) / 64), 0ull);
    for (int64_t i = 0; i < n; i++) {
        const uint64_t v = pixels[i];
        *at = i;
        if (v >= npix) return "an entry outside the frame";
        const uint64_t bit = 1ull << (v & 63);
        if (seen[(size_t)(v >> 6)] & bit) return "a pixel named twice";
        seen[(size_t)(v >> 6)] |= bit;
    }
    return nullptr;
}

} // namespace rtc

extern "C" {

int rt_render_pixels_device(rt_scene* s, const uint32_t* d_pixels, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                            double* d_sum, uint32_t* d_samples, uint32_t* d_misses, double* d_q, uint32_t* d_batches,
                            uint64_t plane, unsigned long long* d_rays, void* stream)
{
    bool empty;
    int rc = check_render_pixels(s, d_pixels, n, spp, d_sum, d_samples, d_misses, d_q, d_batches, "rt_render_pixels_device",
                                 &empty);
    if (rc != RT_OK || empty) return rc;
    const int kernel = s->variant >> 1;
    if (n > render_rays_max_n(kernel, spp)) {
        set_error("rt_render_pixels_device: more entries than one launch's 32-bit work items hold at this spp; split the list");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params_pixels(kernel, n, spp, seed, sample_base, s->params.width, s->params.height);
    rc = run_pixels(s, p, d_pixels, d_rays ? d_rays : s->rays.p, st); // (no count wanted: the scene's scratch word)
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate_pixels(p, d_sum, d_samples, d_misses, d_q, d_batches, (size_t)plane, st));
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) with 4-B entries going up and one PixelRec per entry coming down, folded
// from zero; the host pool adds it into the caller's frame arrays at the entry's pixel (no pixel is named
// twice, so the pool's ranges write disjoint elements).
int rt_render_pixels(rt_scene* s, const uint32_t* pixels, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                     rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches, uint64_t* rays_out)
{
    bool empty;
    int rc = check_render_pixels(s, pixels, n, spp, sum_rgb, samples, misses, q, batches, "rt_render_pixels", &empty);
    if (rc != RT_OK || empty) return rc;
    const int W = s->params.width, H = s->params.height;
    int64_t at = 0;
    if (const char* bad = check_pixel_list(pixels, n, (uint64_t)W * (uint64_t)H, &at)) {
        set_error(std::string("rt_render_pixels: bad argument (") + bad + ", entry " + std::to_string(at) + ")");
        return RT_ERR_ARG;
    }
    const int kernel = s->variant >> 1;
    const int64_t fit = chunk_fit(make_params_pixels(kernel, 64, spp, seed, sample_base, W, H));
    if (fit < 64) {
        set_error("rt_render_pixels: spp too large for one launch; render it in several calls (sample_base)");
        return RT_ERR_ARG;
    }
    uint32_t* stage_list = nullptr;
    ChunkJob job{n, kPixelsChunk, fit, sizeof(PixelRec), sizeof(uint32_t), /*one_piece*/ false, /*count_rays*/ true};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->pixel_list.reserve(2 * C));
        HIP_TRY(s->pixel_recs.reserve(2 * C));
        stage_list = reinterpret_cast<uint32_t*>(up);
        d_down = s->pixel_recs.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        std::memcpy(stage_list + slot, pixels + first, m * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(s->pixel_list.p + slot, stage_list + slot, m * sizeof(uint32_t), hipMemcpyHostToDevice,
                               s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t, size_t m, size_t slot, hipStream_t st) -> int {
        PathParams p = make_params_pixels(kernel, (int64_t)m, spp, seed, sample_base, W, H);
        const int lrc = run_pixels(s, p, s->pixel_list.p + slot, s->rays.p, st);
        if (lrc != RT_OK) return lrc;
        HIP_TRY(launch_accumulate_pixels_recs(p, s->pixel_recs.p + slot, st));
        return RT_OK;
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const PixelRec* r = reinterpret_cast<const PixelRec*>(stage);
        for (size_t i = a; i < b; i++) {
            const uint32_t pix = pixels[first + (i - slot)];
            const size_t o = (size_t)(pix % (uint32_t)W) * (size_t)H + (size_t)(pix / (uint32_t)W);
            sum_rgb[o].r += r[i].r;
            sum_rgb[o].g += r[i].g;
            sum_rgb[o].b += r[i].b;
            samples[o] += r[i].samples;
            misses[o] += r[i].misses;
            if (q) {
                q[o] += r[i].q;
                batches[o] += r[i].batches;
            }
        }
    };
    return run_chunks(s, job, rays_out);
}

} // extern "C"
