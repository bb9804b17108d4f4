// api_render_pixels.hip -- the C ABI's list renders (include/rtcore.h, "adaptive sampling"): the
// camera's own samples of a list of frame pixels, by the PIXELS instances of the path kernels
// (kernels_path.hip, refill), folded into whole-frame accumulators with the moments of the error estimate.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

namespace {

constexpr int64_t kPixelsChunk = 1 << 19;    // entries of one chunk of rt_render_pixels (rt_render_rays' size and variable)
constexpr uint64_t kChunkItems = 1ull << 26; // most work items of one chunk: 1 GiB of 16-B partials

// The path kernel of the scene's variant, PIXELS instance, over the n entries at d_pixels, and nothing
// after it: the caller folds p's partials.  run_rays with the camera and the pixel-key table in the
// rays' place; like it, without what rt_render_pixels leaves alone: no timing slot, no counters, no
// ray log, never the scene-specialised kernel, no block cull.
int run_pixels(rt_scene* s, PathParams& p, const uint32_t* d_pixels, unsigned long long* d_count, hipStream_t stream)
{
    const size_t need = (size_t)p.n_chunks * (size_t)p.n_pad;
    uint64_t tickets = 0;
    for (int g = 0; g < p.n_split; g++) tickets += p.split_tickets[g];
    if (need > 0xF0000000ull || tickets > need / 64) { // (run_path's bound; the entry points check n first)
        set_error("rt_render_pixels: n x spp too large for one launch");
        return RT_ERR_ARG;
    }
    HIP_TRY(s->partial.reserve(need));
    HIP_TRY(s->counter.reserve(kMaxSplit * kSplitStride));
    p.partial = s->partial.p;
    p.counter = s->counter.p;
    p.rays = d_count;
    p.pixel_list = d_pixels;
    p.cull = nullptr;
    if (s->any_op && stream != s->last_stream) HIP_TRY(hipStreamWaitEvent(stream, s->done_ev, 0));
    HIP_TRY(hipMemsetAsync(p.counter, 0, sizeof(unsigned int) * kSplitStride * p.n_split, stream));
    const size_t dyn = path_dyn_lds(s->dev, s->variant);
    if (s->pixels_variant != s->variant) {
        s->pixels_blocks_per_cu = path_blocks_per_cu(s->variant, dyn, false, s->dev.n_vn > 0, ITEMS_PIXELS);
        s->pixels_variant = s->variant;
    }
    int grid = s->n_cu * s->pixels_blocks_per_cu;
    p.pkeys = nullptr;
    if ((s->variant >> 1) < 2) { // a small brute-force launch runs fewer blocks per CU (see run_path)
        const double samples = (double)p.n_rays * (double)p.spp;
        int cap = (int)std::ceil(samples / ((double)s->n_cu * 256.0 * 6.0));
        if (const char* e = getenv("RTCORE_GRID_BPC")) cap = atoi(e);
        grid = s->n_cu * std::min(s->pixels_blocks_per_cu, std::max(1, cap));
        // the scene's pixel-key table, as a tile launch reads it (run_path builds it the same way)
        static const bool pkeys_on = !(getenv("RTCORE_PIXEL_KEYS") && getenv("RTCORE_PIXEL_KEYS")[0] == '0');
        if (pkeys_on) {
            if (!s->pkeys_valid || s->pkeys_seed != p.seed) {
                HIP_TRY(s->pkeys.reserve((size_t)s->params.width * (size_t)s->params.height));
                HIP_TRY(launch_pixel_keys(p.seed_key, s->params.width, s->params.height, s->pkeys.p, stream));
                s->pkeys_valid = true;
                s->pkeys_seed = p.seed;
            }
            p.pkeys = s->pkeys.p;
        }
    } else {
        HIP_TRY(s->stack_ovf.reserve((size_t)grid * 256 * kStackOverflow));
        p.stack_ovf = s->stack_ovf.p;
    }
    fill_launch(s->dev, s->variant, p);
    const PathParams* pa = nullptr;
    const int rc = upload_params(s, p, stream, &pa);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_path(s->dev, s->camf_d.p, pa, s->variant, grid, stream, false, ITEMS_PIXELS));
    return RT_OK;
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

// rt_render_rays' pipeline with 4-B entries going up and one PixelRec per entry coming down: chunk k's
// entries go through pinned staging to device slot k & 1 on copy_stream, its launch runs on the scene's
// stream once they have landed, and its records (folded from zero) come back on copy_stream into the
// staging slot the host pool then adds into the caller's frame arrays at each entry's pixel (no pixel is
// named twice, so the pool's ranges write disjoint elements).
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
    int64_t chunk = kPixelsChunk;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(kPixelsChunk, atoll(e)));
    // a chunk's partials stay below kChunkItems items (whole blocks of 64 entries), whatever spp is
    const PathParams probe = make_params_pixels(kernel, 64, spp, seed, sample_base, W, H);
    const int64_t fit = (int64_t)(kChunkItems / ((uint64_t)probe.n_chunks * 64u)) * 64;
    if (fit < 64) {
        set_error("rt_render_pixels: spp too large for one launch; render it in several calls (sample_base)");
        return RT_ERR_ARG;
    }
    chunk = std::min(std::min(chunk, fit), n);
    HIP_TRY(hipSetDevice(s->device));
    if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamSynchronize(s->copy_stream)); // (copies a failed call left behind: see rt_render_tile)
    const size_t C = (size_t)chunk;
    HIP_TRY(s->pixel_list.reserve(2 * C));
    HIP_TRY(s->pixel_recs.reserve(2 * C));
    // pinned staging: the two record slots (at the offsets queue_copy gives them), then the two list slots
    HIP_TRY(s->stage.reserve(2 * C * (sizeof(PixelRec) + sizeof(uint32_t))));
    HIP_TRY(s->rays_h.reserve(1));
    uint32_t* stage_list = reinterpret_cast<uint32_t*>(s->stage.p + 2 * C * sizeof(PixelRec));
    for (int j = 0; j < 2; j++) {
        if (!s->query_up_ev[j]) HIP_TRY(hipEventCreateWithFlags(&s->query_up_ev[j], hipEventDisableTiming));
        if (!s->band_ev[j]) HIP_TRY(hipEventCreateWithFlags(&s->band_ev[j], hipEventDisableTiming));
    }
    hipStream_t st = s->stream;
    if (s->any_op && st != s->last_stream) HIP_TRY(hipStreamWaitEvent(st, s->done_ev, 0));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), st));
    const int64_t K = (n + chunk - 1) / chunk;
    auto count = [&](int64_t k) { return (size_t)std::min(chunk, n - k * chunk); };
    auto upload = [&](int64_t k) -> int {
        const size_t m = count(k), slot = (size_t)(k & 1) * C;
        std::memcpy(stage_list + slot, pixels + k * chunk, m * sizeof(uint32_t));
        HIP_TRY(hipMemcpyAsync(s->pixel_list.p + slot, stage_list + slot, m * sizeof(uint32_t), hipMemcpyHostToDevice,
                               s->copy_stream));
        HIP_TRY(hipEventRecord(s->query_up_ev[k & 1], s->copy_stream));
        return RT_OK;
    };
    CopyPlan plans[2];
    auto consume = [&](int64_t k) -> int {
        const size_t slot = (size_t)(k & 1) * C, first = (size_t)(k * chunk);
        return consume_copies(s, plans[k & 1], [&](const unsigned char* stage, size_t a, size_t b) {
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
        });
    };
    rc = upload(0);
    if (rc != RT_OK) return rc;
    for (int64_t k = 0; k < K; k++) {
        const size_t m = count(k), slot = (size_t)(k & 1) * C;
        HIP_TRY(hipStreamWaitEvent(st, s->query_up_ev[k & 1], 0));
        PathParams p = make_params_pixels(kernel, (int64_t)m, spp, seed, sample_base, W, H);
        rc = run_pixels(s, p, s->pixel_list.p + slot, s->rays.p, st);
        if (rc != RT_OK) return rc;
        HIP_TRY(launch_accumulate_pixels_recs(p, s->pixel_recs.p + slot, st));
        HIP_TRY(hipEventRecord(s->band_ev[k & 1], st));
        if (k >= 1) {
            rc = consume(k - 1);
            if (rc != RT_OK) return rc;
        }
        if (k + 1 < K) {
            rc = upload(k + 1);
            if (rc != RT_OK) return rc;
        }
        HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->band_ev[k & 1], 0));
        if (k + 1 == K) // (before the last records, so it has landed when they have)
            HIP_TRY(hipMemcpyAsync(s->rays_h.p, s->rays.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->copy_stream));
        plans[k & 1] = CopyPlan{};
        rc = queue_copy(s, plans[k & 1], s->pixel_recs.p, slot, slot + m, sizeof(PixelRec),
                        (int)std::max<size_t>(1, std::min<size_t>(rt_scene::kCopyChunks, (m * sizeof(PixelRec)) >> 20)),
                        s->copy_stream);
        if (rc != RT_OK) return rc;
    }
    rc = end_op(s, st);
    if (rc != RT_OK) return rc;
    rc = consume(K - 1);
    if (rc != RT_OK) return rc;
    if (rays_out) *rays_out += s->rays_h.p[0];
    return RT_OK;
}

} // extern "C"
