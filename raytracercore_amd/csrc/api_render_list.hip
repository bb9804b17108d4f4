// api_render_list.hip -- the C ABI's indexed radiance queries (include/rtcore.h, "indexed radiance
// queries"): rt_render_rays, rt_render_beams or rt_render_surfels for a list of entry numbers into an
// array of records, added into per-entry accumulators with rt_render_pixels' moments.  The launch is
// the three entry points' own (run_rays, api_render_rays.hip) with an index list in the launch record
// (PathParams::index_list, refill's list_entry); the fold is rt_render_pixels' (accumulate_list_kernel).
#include <cstring>

#include "rt_scene.h"

static_assert(sizeof(rt_surfel) == sizeof(rt_ray) && sizeof(rt_beam) == 3 * sizeof(rt_ray), "records in rt_ray units");

namespace {

// The three kinds as the existing entry points describe them (record size, host chunk, name).
bool list_kind(int32_t kind, int32_t gather_mode, RenderList* out)
{
    switch (kind) {
    case RT_LIST_RAYS: *out = RenderList{ITEMS_RAYS, sizeof(rt_ray), 1 << 19, "rays"}; return true;
    case RT_LIST_BEAMS: *out = RenderList{ITEMS_BEAMS, sizeof(rt_beam), 1 << 18, "beams"}; return true;
    case RT_LIST_SURFELS: *out = RenderList{ITEMS_SURFELS, sizeof(rt_surfel), 1 << 19, "surfels", gather_mode}; return true;
    }
    return false;
}

// Every check of both entry points, in the header's order; RT_OK with *empty set for n == 0.
int check_render_list(rt_scene* s, int32_t kind, int32_t gather_mode, const void* records, int64_t n_records,
                      const uint32_t* index, int64_t n, int32_t spp, const void* sum, const void* samples, const void* misses,
                      const void* q, const void* batches, uint64_t plane, const char* name, RenderList* what, bool* empty)
{
    *empty = false;
    const char* bad = nullptr;
    if (!list_kind(kind, gather_mode, what)) {
        bad = "unknown kind";
    } else if (kind == RT_LIST_SURFELS) {
        if (gather_mode != RT_GATHER_DIFFUSE && gather_mode != RT_GATHER_COSINE && gather_mode != RT_GATHER_SPHERE)
            bad = "unknown gather mode";
    } else if (gather_mode != 0) {
        bad = "a gather mode for rays or beams";
    }
    if (!bad) bad = !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && (q != nullptr) != (batches != nullptr)) bad = "q and batches go together";
    if (!bad && n == 0) { // (as rt_render_rays: an empty list may come with null arrays)
        *empty = true;
        return RT_OK;
    }
    if (!bad && (!records || !sum || !samples || !misses)) bad = "null pointer";
    if (!bad && n_records <= 0) bad = "n_records <= 0";
    if (!bad && n_records >= ((int64_t)1 << 32)) bad = "2^32 records or more";
    if (!bad && plane != 0 && plane < (uint64_t)n_records) bad = "plane below n_records";
    if (!bad && !index && n != n_records) bad = "no index list and n != n_records";
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

} // namespace

extern "C" {

int rt_render_list_device(rt_scene* s, int32_t kind, int32_t gather_mode, const void* d_records, int64_t n_records,
                          const uint32_t* d_index, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                          uint64_t stream_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses, double* d_q,
                          uint32_t* d_batches, uint64_t plane, unsigned long long* d_rays_count, void* stream)
{
    RenderList what{};
    bool empty;
    int rc = check_render_list(s, kind, gather_mode, d_records, n_records, d_index, n, spp, d_sum, d_samples, d_misses, d_q,
                               d_batches, plane, "rt_render_list_device", &what, &empty);
    if (rc != RT_OK || empty) return rc;
    const int kernel = s->variant >> 1;
    if (n > render_rays_max_n(kernel, spp)) {
        set_error("rt_render_list_device: more entries than one launch's 32-bit work items hold at this spp; split the list");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params_rays(kernel, n, spp, seed, sample_base, stream_base);
    // (no count wanted: the scene's scratch word)
    rc = run_rays(s, what, p, d_records, d_rays_count ? d_rays_count : s->rays.p, st, d_index, (unsigned)n_records, false);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate_list(p, d_index, (size_t)n_records, d_sum, d_samples, d_misses, d_q, d_batches, (size_t)plane,
                                   nullptr, st));
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) with the listed records gathered on the host: chunk k is the list
// positions [k C, ..); their records go into the chunk's staging slot in list order and their entry
// numbers beside them, both up to device slot k & 1; the launch reads the record at the list position
// and keys the stream by the entry (PathParams::list_gathered), so an entry's samples do not depend on
// the chunking; one PixelRec per list position comes back and the host pool adds it at the entry (no
// entry is named twice, so the pool's ranges write disjoint elements).
// Without an index list the chunk is a run of consecutive entries and needs no list on the device: the
// launch is rt_render_rays' own, keyed from stream_base + k C.
int rt_render_list(rt_scene* s, int32_t kind, int32_t gather_mode, const void* records, int64_t n_records,
                   const uint32_t* index, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base,
                   rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches, uint64_t* rays_out)
{
    RenderList what{};
    bool empty;
    int rc = check_render_list(s, kind, gather_mode, records, n_records, index, n, spp, sum_rgb, samples, misses, q, batches, 0,
                               "rt_render_list", &what, &empty);
    if (rc != RT_OK || empty) return rc;
    int64_t at = 0;
    // rt_render_pixels' bitmap check with the records as the frame (its own words speak of pixels)
    if (index && check_pixel_list(index, n, (uint64_t)n_records, &at)) {
        set_error(std::string("rt_render_list: bad argument (") +
                  (index[at] >= (uint64_t)n_records ? "an entry at or past n_records" : "an entry named twice") + ", entry " +
                  std::to_string(at) + ")");
        return RT_ERR_ARG;
    }
    const int kernel = s->variant >> 1;
    const size_t R = what.rec_bytes / sizeof(rt_ray);
    const rt_ray* recs_in = static_cast<const rt_ray*>(records);
    const int64_t fit = chunk_fit(make_params_rays(kernel, 64, spp, seed, sample_base, stream_base));
    if (fit < 64) {
        set_error("rt_render_list: spp too large for one launch; render it in several calls (sample_base)");
        return RT_ERR_ARG;
    }
    rt_ray* stage_recs = nullptr;
    uint32_t* stage_list = nullptr;
    ChunkJob job{n, what.chunk, fit, sizeof(PixelRec), what.rec_bytes + sizeof(uint32_t), /*one_piece*/ false, /*count_rays*/ true};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C * R));
        HIP_TRY(s->pixel_list.reserve(2 * C));
        HIP_TRY(s->pixel_recs.reserve(2 * C));
        stage_recs = reinterpret_cast<rt_ray*>(up); // the two slots of the caller's records, then the two list slots
        stage_list = reinterpret_cast<uint32_t*>(stage_recs + 2 * C * R);
        d_down = s->pixel_recs.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        rt_ray* dst = stage_recs + slot * R;
        if (index) {
            parallel_ranges(m, 16384, [&](size_t a, size_t b) {
                for (size_t i = a; i < b; i++)
                    std::memcpy(dst + i * R, recs_in + (size_t)index[first + i] * R, R * sizeof(rt_ray));
            });
            std::memcpy(stage_list + slot, index + first, m * sizeof(uint32_t));
            HIP_TRY(hipMemcpyAsync(s->pixel_list.p + slot, stage_list + slot, m * sizeof(uint32_t), hipMemcpyHostToDevice,
                                   s->copy_stream));
        } else {
            const rt_ray* src = recs_in + first * R;
            parallel_ranges(m * R, 65536, [&](size_t a, size_t b) { std::memcpy(dst + a, src + a, (b - a) * sizeof(rt_ray)); });
        }
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot * R, dst, m * R * sizeof(rt_ray), hipMemcpyHostToDevice, s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t first, size_t m, size_t slot, hipStream_t st) -> int {
        PathParams p = make_params_rays(kernel, (int64_t)m, spp, seed, sample_base,
                                        index ? stream_base : stream_base + (uint64_t)first);
        const uint32_t* d_index = index ? s->pixel_list.p + slot : nullptr;
        const int lrc = run_rays(s, what, p, s->query_rays.p + slot * R, s->rays.p, st, d_index, (unsigned)n_records, true);
        if (lrc != RT_OK) return lrc;
        // (from zero, per list position: the fold takes no entry numbers, every entry is inside)
        HIP_TRY(launch_accumulate_list(p, nullptr, m, nullptr, nullptr, nullptr, nullptr, nullptr, 0, s->pixel_recs.p + slot, st));
        return RT_OK;
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const PixelRec* r = reinterpret_cast<const PixelRec*>(stage);
        for (size_t i = a; i < b; i++) {
            const size_t pos = first + (i - slot), o = index ? (size_t)index[pos] : pos;
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
