// api_occluded_surfels.hip -- the C ABI's occlusion counts for surfels (include/rtcore.h, "occlusion
// queries", rt_occluded_surfels): rt_occluded_rays with the sample's direction drawn on the device about
// the surfel's normal (rt_surfel.h) and the answers counted per surfel.  The kernels are
// kernels_query.hip's occluded_surfels_*; here the launch planning (how many launches the 32-bit work
// indices need, the brute-force kernels' sample blocks) and the two entry points.  The host entry runs
// the chunk pipeline in rt_occluded_rays' buffers: a surfel has an rt_ray's size.
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

static_assert(sizeof(rt_surfel) == sizeof(rt_ray), "rt_surfel takes an rt_ray's place in query_rays and the staging");

namespace {

// The work split (DESIGN.md 4.12 has the A/B measurements behind both).
constexpr unsigned kLanesGrouped = 4; // the grouped order: lanes that share a list position when the positions fill the device
constexpr unsigned kRefill = 16;      // BVH: lanes without a query that trigger a refill

bool known_mode(int32_t mode) { return mode == RT_GATHER_DIFFUSE || mode == RT_GATHER_COSINE || mode == RT_GATHER_SPHERE; }

// The argument and state checks of both entry points (n_records and the list: the device entry's);
// RT_OK with *empty set for n == 0.
int check_surfels(rt_scene* s, int32_t gather_mode, const void* surfels, int64_t n_records, bool listed, int64_t n, int32_t spp,
                  const void* occluded, const char* name, bool* empty)
{
    *empty = false;
    const char* bad = !known_mode(gather_mode) ? "unknown gather mode" : !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!bad)
        bad = (!surfels || !occluded)                  ? "null pointer"
              : (n_records <= 0 || n_records >> 32)    ? "n_records <= 0 or >= 2^32"
              : (!listed && n != n_records)            ? "no index list and n != n_records"
                                                       : nullptr;
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": RT_QUERY_FAST runs in the traversal modes BRUTE, GROUPED and BVH; this scene "
                                      "is in BVH2 mode (rt_scene_set_traversal), use RT_TRAVERSAL_BVH or RT_QUERY_EXACT");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// What a call fixes for all of its launches.
struct Draw {
    int32_t gather_mode;
    rt_key2 seed_key;
    uint64_t sample_base, stream_base;
};

// One launch on `st`: list positions [0, n) of d_index (null: entries [0, n) themselves), samples [0, spp)
// from dr.sample_base, n * spp <= kQueryLaunchMax.
int launch_counts(rt_scene* s, const Draw& dr, const rt_surfel* d_surfels, unsigned n_records, const uint32_t* d_index, unsigned n,
                  const double* d_t_max, unsigned spp, uint32_t* d_occluded, uint32_t* d_samples, hipStream_t st)
{
    const int kernel = query_kernel(s);
    const int per_cu = occluded_surfels_blocks_per_cu(kernel);
    OccludedSurfelsParams p{};
    p.block = spp;
    p.blocks = 1;
    p.refill = kRefill;
    if (const char* e = getenv("RTCORE_OCCLUDED_SURFELS_REFILL")) p.refill = (unsigned)std::max(1, std::min(64, atoi(e)));
    uint64_t lanes = (uint64_t)n * spp; // the BVH kernel's units
    if (kernel != 3) {
        // The lanes of a position.  A lane walks its surfel's samples alone and pays for the surfel once;
        // the grouped order spreads them over up to 4 lanes, whose wave then holds fewer surfels for its
        // wave-wide box culling.  Where 64 positions per wave would not even give every SIMD a wave, few
        // positions with many samples, a position takes up to a whole wave.  Always a power of two that
        // spp fills (RTCORE_OCCLUDED_SURFELS_LANES sets another, for A/B).
        const uint64_t want = (uint64_t)s->n_cu * per_cu * 4 * 2;
        unsigned want_lanes = ((uint64_t)n + 63) / 64 < (uint64_t)s->n_cu * 4 ? 64u : kernel == 1 ? kLanesGrouped : 1u;
        if (const char* e = getenv("RTCORE_OCCLUDED_SURFELS_LANES")) want_lanes = (unsigned)std::max(1, std::min(64, atoi(e)));
        want_lanes = std::min(want_lanes, spp);
        while ((2u << p.log2_lanes) <= want_lanes) p.log2_lanes++;
        const unsigned per_pos = 1u << p.log2_lanes;
        // The counts are integers, so the block is free: all of a position's samples in one unit while the
        // units fill the device twice over, else as many sample blocks as do, each a whole number of
        // rounds of the position's lanes (RTCORE_OCCLUDED_SURFELS_BLOCK sets the block's samples, for A/B).
        const uint64_t groups = ((uint64_t)n * per_pos + 63) / 64;
        const unsigned split = (unsigned)std::min<uint64_t>(spp, (want + groups - 1) / groups);
        p.block = (spp + split - 1) / split;
        if (const char* e = getenv("RTCORE_OCCLUDED_SURFELS_BLOCK")) p.block = (unsigned)std::max(1, std::min<int>((int)spp, atoi(e)));
        p.block = (p.block + per_pos - 1) / per_pos * per_pos;
        p.blocks = (spp + p.block - 1) / p.block;
        lanes = groups * p.blocks * 64;
    }
    int grid = 0;
    const int rc = fill_query(s, kernel, per_cu, reinterpret_cast<const rt_ray*>(d_surfels),
                              (unsigned)std::min<uint64_t>(lanes, (uint64_t)kQueryLaunchMax), st, p.q, grid);
    if (rc != RT_OK) return rc;
    p.q.n = n;
    p.index = d_index;
    p.n_records = n_records;
    p.t_max = d_t_max;
    p.occluded = d_occluded;
    p.samples = d_samples;
    p.early = 1; // rt_occluded_rays' order and its switch (launch_segments, api_query.hip)
    if (const char* e = getenv("RTCORE_OCCLUDED_EARLY")) p.early = atoi(e) != 0;
    p.gather_mode = dr.gather_mode;
    p.spp = spp;
    p.seed_key = dr.seed_key;
    p.sample_base = dr.sample_base;
    p.stream_base = dr.stream_base;
    HIP_TRY(launch_occluded_surfels(p, kernel, grid, st));
    return RT_OK;
}

// Every launch of n list positions x spp samples on `st`, after the stream ordering is settled: the
// positions in runs of at most kQueryLaunchMax / spp, and a run of one position in sample ranges of at
// most kQueryLaunchMax.  Without a list a run's entries are its positions: the arrays and the stream
// numbers move with it.
int launch_all(rt_scene* s, const Draw& dr, const rt_surfel* d_surfels, int64_t n_records, const uint32_t* d_index, int64_t n,
               const double* d_t_max, int32_t spp, uint32_t* d_occluded, uint32_t* d_samples, hipStream_t st)
{
    const int64_t run = std::max<int64_t>(1, kQueryLaunchMax / spp), part = std::min<int64_t>(spp, kQueryLaunchMax);
    for (int64_t a = 0; a < n; a += run) {
        const unsigned m = (unsigned)std::min(run, n - a);
        for (int64_t k = 0; k < spp; k += part) {
            Draw d = dr;
            d.sample_base += (uint64_t)k;
            const unsigned kk = (unsigned)std::min<int64_t>(part, spp - k);
            int rc;
            if (d_index) {
                rc = launch_counts(s, d, d_surfels, (unsigned)n_records, d_index + a, m, d_t_max, kk, d_occluded, d_samples, st);
            } else {
                d.stream_base += (uint64_t)a;
                rc = launch_counts(s, d, d_surfels + a, m, nullptr, m, d_t_max ? d_t_max + a : nullptr, kk, d_occluded + a,
                                   d_samples ? d_samples + a : nullptr, st);
            }
            if (rc != RT_OK) return rc;
        }
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_occluded_surfels_device(rt_scene* s, int32_t gather_mode, const rt_surfel* d_surfels, int64_t n_records,
                               const uint32_t* d_index, int64_t n, const double* d_t_max, int32_t spp, uint64_t seed,
                               uint64_t sample_base, uint64_t stream_base, uint32_t* d_occluded, uint32_t* d_samples, void* stream)
{
    bool empty;
    int rc = check_surfels(s, gather_mode, d_surfels, n_records, d_index != nullptr, n, spp, d_occluded,
                           "rt_occluded_surfels_device", &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    // the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    const Draw dr{gather_mode, rt_rng_seed_key(seed), sample_base, stream_base};
    rc = launch_all(s, dr, d_surfels, n_records, d_index, n, d_t_max, spp, d_occluded, d_samples, st);
    if (rc != RT_OK) return rc;
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) with 72 B up (64 B without t_max) and 4 B down per surfel, for any spp:
// the surfels' two staging slots, then the two slots of segment ends.  A chunk's counts are zeroed on the
// scene's stream before its kernel adds to them (after the download that last read the slot: the
// kernel's wait for its upload orders that), and the host adds them, and spp, into the caller's arrays.
int rt_occluded_surfels(rt_scene* s, int32_t gather_mode, const rt_surfel* surfels, int64_t n, const double* t_max, int32_t spp,
                        uint64_t seed, uint64_t sample_base, uint64_t stream_base, uint32_t* occluded, uint32_t* samples)
{
    bool empty;
    int rc = check_surfels(s, gather_mode, surfels, 1, true, n, spp, occluded, "rt_occluded_surfels", &empty); // (no list, any n)
    if (rc != RT_OK || empty) return rc;
    const Draw dr{gather_mode, rt_rng_seed_key(seed), sample_base, stream_base};
    rt_surfel* stage_surfels = nullptr;
    double* stage_t = nullptr;
    ChunkJob job{n, kQueryChunk, 0, sizeof(uint32_t), sizeof(rt_surfel) + sizeof(double), /*one_piece*/ true,
                 /*count_rays*/ false};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C));
        HIP_TRY(s->occluded_counts.reserve(2 * C));
        if (t_max) HIP_TRY(s->occluded_t_max.reserve(2 * C));
        stage_surfels = reinterpret_cast<rt_surfel*>(up);
        stage_t = reinterpret_cast<double*>(stage_surfels + 2 * C);
        d_down = s->occluded_counts.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        const rt_surfel* src = surfels + first;
        const double* src_t = t_max ? t_max + first : nullptr;
        parallel_ranges(m, 65536, [&](size_t a, size_t b) {
            std::memcpy(stage_surfels + slot + a, src + a, (b - a) * sizeof(rt_surfel));
            if (src_t) std::memcpy(stage_t + slot + a, src_t + a, (b - a) * sizeof(double));
        });
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot, stage_surfels + slot, m * sizeof(rt_surfel), hipMemcpyHostToDevice,
                               s->copy_stream));
        if (src_t)
            HIP_TRY(hipMemcpyAsync(s->occluded_t_max.p + slot, stage_t + slot, m * sizeof(double), hipMemcpyHostToDevice,
                                   s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t first, size_t m, size_t slot, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s->occluded_counts.p + slot, 0, m * sizeof(uint32_t), st));
        Draw d = dr;
        d.stream_base += (uint64_t)first;
        return launch_all(s, d, reinterpret_cast<const rt_surfel*>(s->query_rays.p + slot), (int64_t)m, nullptr, (int64_t)m,
                          t_max ? s->occluded_t_max.p + slot : nullptr, spp, s->occluded_counts.p + slot, nullptr, st);
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const uint32_t* c = reinterpret_cast<const uint32_t*>(stage);
        for (size_t i = a; i < b; i++) {
            occluded[first + (i - slot)] += c[i];
            if (samples) samples[first + (i - slot)] += (uint32_t)spp;
        }
    };
    return run_chunks(s, job);
}

} // extern "C"
