// api_render_probes.hip -- the C ABI's light probes (include/rtcore.h, "light probes", rt_probe_sh): per
// point, the sums of its RT_GATHER_SPHERE gather samples weighted by the nine L2 spherical-harmonic basis
// functions of each sample's direction.  A probe launch is rt_render_surfels' own (run_rays over the SURFELS
// instances of the path kernels, untouched) planned with one sample per work item (make_params_probes), so
// that a partial row is one sample; accumulate_probes_kernel (kernels_fold.hip) draws each sample's direction
// again and folds the rows in sample order.  Here: the two entry points and the host twins of the basis and
// of the fold, second compilations of rt_sh.h.
#include <cstring>

#include "rt_scene.h"
#include "rt_sh.h"

static_assert(sizeof(rt_probe_sh) == 288 && sizeof(ProbeRec) == sizeof(rt_probe_sh) + 8, "rt_probe_sh: nine rows of four doubles");

namespace {

constexpr int64_t kProbesChunk = 1 << 19; // probes of one chunk of rt_render_probes (rt_render_surfels' size and variable)
constexpr RenderList kProbes = {ITEMS_SURFELS, sizeof(rt_surfel), kProbesChunk, "probes", RT_GATHER_SPHERE};

} // namespace

extern "C" {

int rt_render_probes_device(rt_scene* s, const rt_surfel* d_probes, int64_t n, int32_t spp, uint64_t seed,
                            uint64_t sample_base, uint64_t stream_base, rt_probe_sh* d_sh, uint32_t* d_samples,
                            uint32_t* d_misses, unsigned long long* d_count, void* stream)
{
    const char* name = "rt_render_probes_device";
    bool empty;
    int rc = check_render_rays(s, d_probes, n, spp, d_sh, d_samples, d_misses, name, &empty);
    if (rc != RT_OK || empty) return rc;
    if (n > probes_max_n(spp)) {
        set_error(std::string(name) + ": 64 * ceil(n / 64) * (spp rounded up to a power of two) is above one launch's 2^26 "
                                      "work items; split the call by n or by sample_base");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params_probes(s->variant >> 1, n, spp, seed, sample_base, stream_base);
    // (no count wanted: the scene's scratch word)
    rc = run_rays(s, kProbes, p, d_probes, d_count ? d_count : s->rays.p, st, nullptr, 0, false);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate_probes(p, d_sh, d_samples, d_misses, nullptr, st));
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) as render_list_host runs it, but for the answers: the sums continue from
// what the caller's arrays hold, in sample order (rtcore.h, promise 3), so a chunk's ProbeRecs go up with
// those values beside the records, the fold adds into them in place, and they come down to replace the
// caller's; only the counts are added here.  Upload k + 1 of a ProbeRec slot follows download k - 1 of it on
// the copy stream, as for every two-chunk buffer.
int rt_render_probes(rt_scene* s, const rt_surfel* probes, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                     uint64_t stream_base, rt_probe_sh* sh, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    const char* name = "rt_render_probes";
    bool empty;
    int rc = check_render_rays(s, probes, n, spp, sh, samples, misses, name, &empty);
    if (rc != RT_OK || empty) return rc;
    if (probes_max_n(spp) < 64) {
        set_error(std::string(name) + ": spp too large for one launch; render it in several calls (sample_base)");
        return RT_ERR_ARG;
    }
    const int kernel = s->variant >> 1;
    const int64_t fit = chunk_fit(make_params_probes(kernel, 64, spp, seed, sample_base, stream_base));
    rt_surfel* stage_probes = nullptr;
    ProbeRec* stage_recs = nullptr;
    ChunkJob job{n, kProbesChunk, fit, sizeof(ProbeRec), sizeof(rt_surfel) + sizeof(ProbeRec), /*one_piece*/ false,
                 /*count_rays*/ true};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C));
        HIP_TRY(s->probe_recs.reserve(2 * C));
        stage_probes = reinterpret_cast<rt_surfel*>(up); // 2 C records, then 2 C ProbeRecs (both 8-byte aligned)
        stage_recs = reinterpret_cast<ProbeRec*>(up + 2 * C * sizeof(rt_surfel));
        d_down = s->probe_recs.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        parallel_ranges(m, 16384, [&](size_t a, size_t b) {
            std::memcpy(stage_probes + slot + a, probes + first + a, (b - a) * sizeof(rt_surfel));
            for (size_t i = a; i < b; i++) {
                stage_recs[slot + i].sh = sh[first + i];
                stage_recs[slot + i].samples = stage_recs[slot + i].misses = 0;
            }
        });
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot, stage_probes + slot, m * sizeof(rt_surfel), hipMemcpyHostToDevice,
                               s->copy_stream));
        HIP_TRY(hipMemcpyAsync(s->probe_recs.p + slot, stage_recs + slot, m * sizeof(ProbeRec), hipMemcpyHostToDevice,
                               s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t first, size_t m, size_t slot, hipStream_t st) -> int {
        PathParams p = make_params_probes(kernel, (int64_t)m, spp, seed, sample_base, stream_base + (uint64_t)first);
        const int lrc = run_rays(s, kProbes, p, s->query_rays.p + slot, s->rays.p, st, nullptr, 0, false);
        if (lrc != RT_OK) return lrc;
        HIP_TRY(launch_accumulate_probes(p, nullptr, nullptr, nullptr, s->probe_recs.p + slot, st));
        return RT_OK;
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const ProbeRec* r = reinterpret_cast<const ProbeRec*>(stage);
        for (size_t i = a; i < b; i++) {
            const size_t o = first + (i - slot);
            sh[o] = r[i].sh;
            samples[o] += r[i].samples;
            misses[o] += r[i].misses;
        }
    };
    return run_chunks(s, job, rays_out);
}

int rt_debug_sh_basis(const double* dirs_xyz, int64_t n, double* y9_out)
{
    if (n < 0 || (n > 0 && (!dirs_xyz || !y9_out))) {
        set_error("rt_debug_sh_basis: bad argument (null pointer or n < 0)");
        return RT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++) sh_basis(dirs_xyz[3 * i], dirs_xyz[3 * i + 1], dirs_xyz[3 * i + 2], y9_out + kShCoeffs * i);
    return RT_OK;
}

int rt_debug_probe_fold(const rt_ray* rays, const float* rgb, const uint8_t* miss, int64_t n, int32_t spp, rt_probe_sh* sh,
                        uint32_t* samples, uint32_t* misses)
{
    if (n < 0 || spp <= 0 || (n > 0 && (!rays || !rgb || !miss || !sh || !samples || !misses))) {
        set_error("rt_debug_probe_fold: bad argument (null pointer, n < 0 or spp <= 0)");
        return RT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++)
        for (int64_t at = i * spp; at < (i + 1) * spp; at++) {
            const rt_vec4d& d = rays[at].direction;
            if (d.x == 0.0 && d.y == 0.0 && d.z == 0.0) { // a sample of an invalid probe: a miss in no direction
                misses[i]++;
                continue;
            }
            double Y[kShCoeffs];
            sh_basis(d.x, d.y, d.z, Y);
            if (miss[at]) {
                misses[i]++;
                for (int l = 0; l < kShCoeffs; l++) sh[i].c[l][3] = sh_add(sh[i].c[l][3], Y[l]);
            } else {
                samples[i]++;
                for (int l = 0; l < kShCoeffs; l++)
                    for (int j = 0; j < 3; j++) sh[i].c[l][j] = sh_add(sh[i].c[l][j], sh_mul((double)rgb[3 * at + j], Y[l]));
            }
        }
    return RT_OK;
}

} // extern "C"
