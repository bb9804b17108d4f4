// api_render_rays.hip -- the C ABI's radiance queries (include/rtcore.h, "radiance queries"):
// Raytracer.GetColor(ray) (Raytracer.cs:248-252) for rays the caller brings, by the RAYS instances of
// the path kernels (kernels_path.hip, refill), accumulated as SampleSet accumulates a pixel.  The
// launch, the argument check and the two entry points' bodies serve rt_render_beams and
// rt_render_surfels as well (api_render_beams.hip, api_render_surfels.hip; the BEAMS and SURFELS
// instances): a RenderList says which records a list holds.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

namespace {

constexpr int64_t kRaysChunk = 1 << 19; // rays of one chunk of rt_render_rays (rt_query_rays' size and variable)
constexpr RenderList kRays = {ITEMS_RAYS, sizeof(rt_ray), kRaysChunk, "rays"};

} // namespace

namespace rtc {

// Argument and state checks shared by both entry points; RT_OK with *empty set for n == 0.
int check_render_rays(rt_scene* s, const void* rays, int64_t n, int32_t spp, const void* sum, const void* samples,
                      const void* misses, const char* name, bool* empty)
{
    *empty = false;
    const char* bad = !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) { // (as rt_query_rays: an empty list may come with null arrays)
        *empty = true;
        return RT_OK;
    }
    if (!bad && (!rays || !sum || !samples || !misses)) bad = "null pointer";
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": runs in the traversal modes BRUTE, GROUPED and BVH; this scene is in BVH2 mode "
                                      "(rt_scene_set_traversal), use RT_TRAVERSAL_BVH");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// The path kernel of the scene's variant, src's instance, and nothing after it: the caller folds p's
// partials.  run_path without what the list renders leave alone: no timing slot, no counters, no ray log,
// never the scene-specialised kernel, no block cull.
int run_items(rt_scene* s, ItemSource src, const char* what, PathParams& p, unsigned long long* d_count, hipStream_t stream)
{
    const size_t need = (size_t)p.n_chunks * (size_t)p.n_pad;
    uint64_t tickets = 0;
    for (int g = 0; g < p.n_split; g++) tickets += p.split_tickets[g];
    if (need > 0xF0000000ull || tickets > need / 64) { // (run_path's bound; the entry points check n first)
        set_error(std::string("rt_render_") + what + ": n x spp too large for one launch");
        return RT_ERR_ARG;
    }
    HIP_TRY(s->partial.reserve(need));
    HIP_TRY(s->counter.reserve(kMaxSplit * kSplitStride));
    p.partial = s->partial.p;
    p.counter = s->counter.p;
    p.rays = d_count;
    HIP_TRY(wait_last_op(s, stream));
    HIP_TRY(hipMemsetAsync(p.counter, 0, sizeof(unsigned int) * kSplitStride * p.n_split, stream));
    const size_t dyn = path_dyn_lds(s->dev, s->variant);
    int& blocks_per_cu = s->items_blocks_per_cu[src];
    if (s->items_variant[src] != s->variant) {
        blocks_per_cu = path_blocks_per_cu(s->variant, dyn, false, s->dev.n_vn > 0, src);
        s->items_variant[src] = s->variant;
    }
    int grid = s->n_cu * blocks_per_cu;
    if (src == ITEMS_PIXELS) p.pkeys = nullptr;
    if ((s->variant >> 1) < 2) { // a small brute-force launch runs fewer blocks per CU (see run_path)
        const double samples = (double)p.n_rays * (double)p.spp;
        int cap = (int)std::ceil(samples / ((double)s->n_cu * 256.0 * 6.0));
        if (const char* e = getenv("RTCORE_GRID_BPC")) cap = atoi(e);
        grid = s->n_cu * std::min(blocks_per_cu, std::max(1, cap));
        // the scene's pixel-key table, as a tile launch reads it (run_path builds it the same way)
        static const bool pkeys_on = !(getenv("RTCORE_PIXEL_KEYS") && getenv("RTCORE_PIXEL_KEYS")[0] == '0');
        if (src == ITEMS_PIXELS && pkeys_on) {
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
    HIP_TRY(launch_path(s->dev, s->camf_d.p, pa, s->variant, grid, stream, false, src));
    return RT_OK;
}

// d_index (rt_render_list; null for the three entry points here): the launch's index list over n_records
// records, gathered as PathParams::list_gathered says.
int run_rays(rt_scene* s, const RenderList& kind, PathParams& p, const void* d_list, unsigned long long* d_count,
             hipStream_t stream, const uint32_t* d_index, unsigned n_records, bool gathered)
{
    p.ray_list = reinterpret_cast<const double2*>(d_list); // (beam_list is the same storage)
    p.gather_mode = kind.gather_mode;                      // (start_rows' word: 0 but for the surfels)
    p.index_list = d_index;                                // (the cull's word: a list launch has none)
    p.n_records = d_index ? n_records : 0u;
    p.list_gathered = d_index && gathered ? 1 : 0;
    return run_items(s, kind.src, kind.what, p, d_count, stream);
}

int render_list_device(rt_scene* s, const RenderList& kind, const char* name, const void* d_list, int64_t n, int32_t spp,
                       uint64_t seed, uint64_t sample_base, uint64_t stream_base, double* d_sum, uint32_t* d_samples,
                       uint32_t* d_misses, unsigned long long* d_count, void* stream)
{
    bool empty;
    int rc = check_render_rays(s, d_list, n, spp, d_sum, d_samples, d_misses, name, &empty);
    if (rc != RT_OK || empty) return rc;
    const int kernel = s->variant >> 1;
    if (n > render_rays_max_n(kernel, spp)) {
        set_error(std::string(name) + ": more " + kind.what +
                  " than one launch's 32-bit work items hold at this spp; split the list");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params_rays(kernel, n, spp, seed, sample_base, stream_base);
    // (no count wanted: the scene's scratch word)
    rc = run_rays(s, kind, p, d_list, d_count ? d_count : s->rays.p, st, nullptr, 0, false);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate_rays(p, d_sum, d_samples, d_misses, nullptr, st));
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) with a path launch and its fold as the chunk's kernels: one TileRec per
// record comes down, folded from zero, and the host pool adds it into the caller's arrays.  The partials
// are one buffer: launch k + 1 follows fold k on the scene's stream.  A record of the list takes R =
// rec_bytes / sizeof(rt_ray) entries of query_rays and of the staging's ray slots (a beam: 3).
int render_list_host(rt_scene* s, const RenderList& kind, const char* name, const void* list, int64_t n, int32_t spp,
                     uint64_t seed, uint64_t sample_base, uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples,
                     uint32_t* misses, uint64_t* rays_out)
{
    bool empty;
    int rc = check_render_rays(s, list, n, spp, sum_rgb, samples, misses, name, &empty);
    if (rc != RT_OK || empty) return rc;
    const int kernel = s->variant >> 1;
    const size_t R = kind.rec_bytes / sizeof(rt_ray);
    const rt_ray* rays = static_cast<const rt_ray*>(list);
    const int64_t fit = chunk_fit(make_params_rays(kernel, 64, spp, seed, sample_base, stream_base));
    if (fit < 64) {
        set_error(std::string(name) + ": spp too large for one launch; render it in several calls (sample_base)");
        return RT_ERR_ARG;
    }
    rt_ray* stage_rays = nullptr;
    ChunkJob job{n, kind.chunk, fit, sizeof(TileRec), kind.rec_bytes, /*one_piece*/ false, /*count_rays*/ true};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C * R));
        HIP_TRY(s->render_rays_recs.reserve(2 * C));
        stage_rays = reinterpret_cast<rt_ray*>(up);
        d_down = s->render_rays_recs.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int { // (m and slot in rt_ray entries from here)
        m *= R, slot *= R;
        const rt_ray* src = rays + first * R;
        parallel_ranges(m, 65536,
                        [&](size_t a, size_t b) { std::memcpy(stage_rays + slot + a, src + a, (b - a) * sizeof(rt_ray)); });
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot, stage_rays + slot, m * sizeof(rt_ray), hipMemcpyHostToDevice,
                               s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t first, size_t m, size_t slot, hipStream_t st) -> int {
        PathParams p = make_params_rays(kernel, (int64_t)m, spp, seed, sample_base, stream_base + (uint64_t)first);
        const int lrc = run_rays(s, kind, p, s->query_rays.p + slot * R, s->rays.p, st, nullptr, 0, false);
        if (lrc != RT_OK) return lrc;
        HIP_TRY(launch_accumulate_rays(p, nullptr, nullptr, nullptr, s->render_rays_recs.p + slot, st));
        return RT_OK;
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const TileRec* r = reinterpret_cast<const TileRec*>(stage);
        for (size_t i = a; i < b; i++) {
            const size_t o = first + (i - slot);
            sum_rgb[o].r += r[i].r;
            sum_rgb[o].g += r[i].g;
            sum_rgb[o].b += r[i].b;
            samples[o] += r[i].samples;
            misses[o] += r[i].misses;
        }
    };
    return run_chunks(s, job, rays_out);
}

} // namespace rtc

extern "C" {

int rt_render_rays_device(rt_scene* s, const rt_ray* d_rays, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                          uint64_t stream_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                          unsigned long long* d_count, void* stream)
{
    return render_list_device(s, kRays, "rt_render_rays_device", d_rays, n, spp, seed, sample_base, stream_base, d_sum,
                              d_samples, d_misses, d_count, stream);
}

int rt_render_rays(rt_scene* s, const rt_ray* rays, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                   uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    return render_list_host(s, kRays, "rt_render_rays", rays, n, spp, seed, sample_base, stream_base, sum_rgb, samples,
                            misses, rays_out);
}

} // extern "C"
