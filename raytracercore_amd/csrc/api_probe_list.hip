// api_probe_list.hip -- the C ABI's adaptive light probes (include/rtcore.h, "adaptive light probes"):
// rt_render_probes_device for a list of entry numbers into a resident probe array, with the second moments of
// each probe's band-0/1 luminance coefficients, and the selection pass that turns those into the next list.
// The launch is rt_render_probes' plan (make_params_probes: one sample per work item) through run_rays with an
// index list in the launch record, as rt_render_list_device's; refill's list_entry reads only the list, the
// record count and item_ray's list position, and set_item_order only chunks, pool and ranges, so neither
// cares that the chunks are not make_params_rays'.  The fold is accumulate_probe_list_kernel
// (kernels_fold.hip).  The selection pass shares rt_adaptive_select_device's scan and scratch
// (select_scan.h).  Here too: the host twins, second compilations of rt_probe_error.h.
#include <cmath>
#include <limits>

#include "rt_probe_error.h"
#include "rt_scene.h"
#include "select_scan.h"

static_assert(sizeof(rt_probe_moments) == 64 && sizeof(rt_probe_select_params) == 48, "rtcore.h: adaptive light probes");

namespace {

constexpr RenderList kProbeList = {ITEMS_SURFELS, sizeof(rt_surfel), 1 << 19, "probe_list", RT_GATHER_SPHERE};

struct ProbeSelectArgs {
    rt_probe_select_params P;
    const rt_probe_sh* sh;
    const uint32_t* samples;
    const uint32_t* misses;
    const rt_probe_moments* moments;
    unsigned n_records;
    int n_blocks;
};

// One wave per 64 consecutive entries (four per workgroup): the block's active lanes as a ballot mask, and
// their number.
__global__ void __launch_bounds__(256) probe_count_kernel(ProbeSelectArgs A, unsigned long long* masks, unsigned int* counts)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= A.n_blocks) return; // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const unsigned e = (unsigned)b * 64u + (unsigned)lane; // (n_records < 2^32, so b < 2^26: no wrap)
    bool act = false;
    if (e < A.n_records)
        act = probe_active(A.P, &A.sh[e].c[0][0], A.samples[e], A.misses[e], &A.moments[e].m[0][0]);
    const unsigned long long m = __ballot(act);
    if (lane == 0) {
        masks[b] = m;
        counts[b] = (unsigned)__popcll(m);
    }
}

// The write: block b's active entries, in lane order, at offs[b] + the lane's rank in the mask; entries at or
// past cap are dropped.
__global__ void __launch_bounds__(256) probe_write_kernel(int n_blocks, const unsigned long long* masks,
                                                          const unsigned int* offs, uint32_t* list, uint32_t cap)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long m = masks[b];
    if (!((m >> lane) & 1ull)) return;
    const unsigned int at = offs[b] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (at >= cap) return;
    list[at] = (uint32_t)b * 64u + (uint32_t)lane;
}

int check_probe_select(const char* name, const rt_probe_select_params* P, const void* sh, const void* samples,
                       const void* misses, const void* moments, int64_t n_records, const void* list, uint32_t cap)
{
    const char* bad = nullptr;
    if (!P || !sh || !samples || !misses || !moments || (!list && cap > 0)) bad = "null pointer";
    else if (n_records <= 0) bad = "n_records <= 0";
    else if (n_records >= ((int64_t)1 << 32)) bad = "2^32 probes or more";
    else if (!(P->rel_tol >= 0.0)) bad = "rel_tol negative or NaN";
    else if (!(P->irr_floor > 0.0)) bad = "irr_floor not above 0";
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_render_probe_list_device(rt_scene* s, const rt_surfel* d_probes, int64_t n_records, const uint32_t* d_index, int64_t n,
                                int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base, rt_probe_sh* d_sh,
                                uint32_t* d_samples, uint32_t* d_misses, rt_probe_moments* d_moments,
                                unsigned long long* d_count, void* stream)
{
    const char* name = "rt_render_probe_list_device";
    bool empty;
    int rc = check_render_rays(s, d_probes, n, spp, d_sh, d_samples, d_misses, name, &empty);
    if (rc != RT_OK || empty) return rc;
    const char* bad = n_records <= 0                       ? "n_records <= 0"
                      : n_records >= ((int64_t)1 << 32)    ? "2^32 records or more"
                      : !d_index && n != n_records         ? "no index list and n != n_records"
                                                           : nullptr;
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    if (n > probes_max_n(spp)) {
        set_error(std::string(name) + ": 64 * ceil(n / 64) * (spp rounded up to a power of two) is above one launch's 2^26 "
                                      "work items; split the list or the call by sample_base");
        return RT_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    PathParams p = make_params_probes(s->variant >> 1, n, spp, seed, sample_base, stream_base);
    // (no count wanted: the scene's scratch word)
    rc = run_rays(s, kProbeList, p, d_probes, d_count ? d_count : s->rays.p, st, d_index, (unsigned)n_records, false);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate_probe_list(p, d_index, (size_t)n_records, d_sh, d_samples, d_misses, d_moments, st));
    return end_op(s, st);
}

int rt_debug_probe_moments(const rt_ray* rays, const float* rgb, const uint8_t* miss, int64_t n, int32_t spp,
                           rt_probe_moments* moments)
{
    if (n < 0 || spp <= 0 || (n > 0 && (!rays || !rgb || !miss || !moments))) {
        set_error("rt_debug_probe_moments: bad argument (null pointer, n < 0 or spp <= 0)");
        return RT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++) {
        double m0[kProbeMomentRows], m1[kProbeMomentRows];
        for (int l = 0; l < kProbeMomentRows; l++) {
            m0[l] = moments[i].m[l][0];
            m1[l] = moments[i].m[l][1];
        }
        for (int64_t at = i * spp; at < (i + 1) * spp; at++) {
            const rt_vec4d& d = rays[at].direction;
            if (d.x == 0.0 && d.y == 0.0 && d.z == 0.0) continue; // a sample of an invalid probe
            double Y[kShCoeffs];
            sh_basis(d.x, d.y, d.z, Y);
            if (miss[at]) probe_moments_miss(m1, Y);
            else probe_moments_hit(m0, rgb[3 * at], rgb[3 * at + 1], rgb[3 * at + 2], Y);
        }
        for (int l = 0; l < kProbeMomentRows; l++) {
            moments[i].m[l][0] = m0[l];
            moments[i].m[l][1] = m1[l];
        }
    }
    return RT_OK;
}

int rt_probe_select_device(const rt_probe_select_params* P, const rt_probe_sh* d_sh, const uint32_t* d_samples,
                           const uint32_t* d_misses, const rt_probe_moments* d_moments, int64_t n_records, uint32_t* d_list,
                           uint32_t cap, uint32_t* d_count, void* stream)
{
    const char* name = "rt_probe_select_device";
    int rc = check_probe_select(name, P, d_sh, d_samples, d_misses, d_moments, n_records, d_list, cap);
    if (rc != RT_OK) return rc;
    if (!d_count) {
        set_error(std::string(name) + ": bad argument (null pointer)");
        return RT_ERR_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProbeSelectArgs A{*P, d_sh, d_samples, d_misses, d_moments, (unsigned)n_records, (int)((n_records + 63) / 64)};
    SelectPass pass;
    rc = select_begin(name, (size_t)A.n_blocks, st, pass);
    if (rc != RT_OK) return rc;
    const unsigned grid = (unsigned)((A.n_blocks + 3) / 4);
    hipLaunchKernelGGL(probe_count_kernel, dim3(grid), dim3(256), 0, st, A, pass.S->masks, pass.S->counts);
    select_scan(pass, A.n_blocks, d_count, st);
    if (cap > 0)
        hipLaunchKernelGGL(probe_write_kernel, dim3(grid), dim3(256), 0, st, A.n_blocks, pass.S->masks, pass.S->counts, d_list,
                           cap);
    return select_end(pass, st);
}

int64_t rt_debug_probe_select(const rt_probe_select_params* P, const rt_probe_sh* sh, const uint32_t* samples,
                              const uint32_t* misses, const rt_probe_moments* moments, int64_t n_records, uint32_t* list,
                              uint32_t cap)
{
    const int rc = check_probe_select("rt_debug_probe_select", P, sh, samples, misses, moments, n_records, list, cap);
    if (rc != RT_OK) return rc;
    int64_t n = 0;
    for (int64_t e = 0; e < n_records; e++) {
        if (!probe_active(*P, &sh[e].c[0][0], samples[e], misses[e], &moments[e].m[0][0])) continue;
        if (n < (int64_t)cap) list[n] = (uint32_t)e;
        n++;
    }
    return n;
}

int rt_debug_probe_error(const rt_probe_select_params* P, const rt_probe_sh* sh, const uint32_t* samples,
                         const uint32_t* misses, const rt_probe_moments* moments, int64_t n, double* se_out, double* level_out)
{
    if (!P || n < 0 || (n > 0 && (!sh || !samples || !misses || !moments || !se_out || !level_out))) {
        set_error("rt_debug_probe_error: bad argument (null pointer or n < 0)");
        return RT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++) {
        const uint64_t N = (uint64_t)samples[i] + (uint64_t)misses[i];
        se_out[i] = level_out[i] = std::numeric_limits<double>::quiet_NaN();
        if (N >= 2) probe_error(P->ambient, &sh[i].c[0][0], &moments[i].m[0][0], (double)N, se_out[i], level_out[i]);
    }
    return RT_OK;
}

} // extern "C"
