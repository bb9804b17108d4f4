// api_probe_depth.hip -- the C ABI's probe depth maps (include/rtcore.h, "probe depth maps", rt_probe_depth):
// per probe an 8 x 8 octahedral map of the moments of the distance its gather samples see, and the shading of
// a probe grid whose corners are weighed by a Chebyshev test against those maps instead of by any-hit rays.
// Three kernels (fold, close, shade) and their host twins, all compilations of rt_probe_depth.h.  The bake's
// chunk is rt_debug_surfel_rays_device's launch (launch_surfel_rays, api_render_surfels.hip) into the scene's
// scratch, rt_query_rays_device's closest-hit launch (launch_rays, api_query.hip) over those rays, and the
// fold; the close and the shading need no scene.
#include <cstdlib>
#include <cstring>

#include "rt_probe_depth.h"
#include "rt_scene.h"

static_assert(sizeof(rt_probe_depth_params) == 32, "rt_probe_depth_params: two 16-byte rows");
static_assert(sizeof(rt_probe_depth) == 3 * kDepthTexels * sizeof(double), "rt_probe_depth: three rows of 64 doubles");
static_assert(sizeof(rt_hit) == 48 && sizeof(rt_ray) == 64, "the bake's scratch: 64 + 48 B per sample");

namespace {

constexpr int32_t kDepthMaxSpp = 1 << 19; // one probe's samples are one chunk at the most
constexpr int kFoldWaves = 4;             // probes per block of the fold kernel

// One wave per probe, lane t owns texel t and walks the probe's samples in order with its three sums in
// registers; no lane reads another's, so the order of the sums is the definition's.  The probe's number is
// made wave-uniform (readfirstlane), so a sample's direction and hit are read through a uniform index: scalar
// loads, shared by the 64 lanes, into the operands of the lanes' fp64 arithmetic.
__global__ void __launch_bounds__(64 * kFoldWaves) probe_depth_fold_kernel(const rt_ray* __restrict__ rays, const rt_hit* __restrict__ hits,
                                                                           unsigned n, unsigned spp, double d_max, int sharpness,
                                                                           rt_probe_depth* __restrict__ depth,
                                                                           uint32_t* __restrict__ counts)
{
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned i = blockIdx.x * (unsigned)kFoldWaves + wave;
    if (i >= n) return;
    const int t = (int)(threadIdx.x & 63u);
    double Tx, Ty, Tz;
    oct_texel_dir(t, Tx, Ty, Tz);
    rt_probe_depth& acc = depth[i];
    double s0 = acc.s[0][t], s1 = acc.s[1][t], s2 = acc.s[2][t];
    unsigned n_hit = 0, n_inside = 0, n_miss = 0, n_skip = 0;
    const rt_ray* __restrict__ r = rays + (size_t)i * spp;
    const rt_hit* __restrict__ h = hits + (size_t)i * spp;
    for (unsigned k = 0; k < spp; k++) {
        const double x = r[k].direction.x, y = r[k].direction.y, z = r[k].direction.z;
        if (x == 0.0 && y == 0.0 && z == 0.0) { // a sample of an invalid probe
            n_skip++;
            continue;
        }
        const bool hit = h[k].prim_id >= 0;
        n_hit += hit ? 1u : 0u;
        n_inside += hit && h[k].inside != 0 ? 1u : 0u;
        n_miss += hit ? 0u : 1u;
        depth_add(Tx, Ty, Tz, x, y, z, depth_of(hit, h[k].distance, d_max), sharpness, s0, s1, s2);
    }
    acc.s[0][t] = s0;
    acc.s[1][t] = s1;
    acc.s[2][t] = s2;
    if (t < 4) counts[(size_t)i * 4 + t] += t == 0 ? n_hit : t == 1 ? n_inside : t == 2 ? n_miss : n_skip;
}

// One thread per texel: three coalesced 8-byte loads, one 16-byte store.
__global__ void __launch_bounds__(256) probe_depth_close_kernel(const rt_probe_depth* __restrict__ depth, unsigned n_texels,
                                                                double2* __restrict__ D)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_texels) return;
    const rt_probe_depth& a = depth[j >> 6];
    const unsigned t = j & 63u;
    double mu, m2;
    depth_close(a.s[0][t], a.s[1][t], a.s[2][t], mu, m2);
    D[j] = make_double2(mu, m2);
}

// One thread per point, as probe_blend_kernel and for its reasons: the 27 sums stay in the
// point's registers and the corners are visited in the definition's order.
__global__ void __launch_bounds__(256) probe_depth_shade_kernel(rt_probe_grid G, rt_probe_depth_params P, const double* __restrict__ L,
                                                                const double* __restrict__ D, const rt_surfel* __restrict__ points,
                                                                unsigned n, rt_color* __restrict__ irradiance,
                                                                double* __restrict__ weight)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rt_surfel s = points[i];
    const ProbeCell c = probe_cell(G, s);
    double E[3], W;
    depth_blend(G, P, L, D, s, c, E, W);
    irradiance[i] = rt_color{E[0], E[1], E[2]};
    if (weight) weight[i] = W;
}

int bad_argument(const char* name, const char* what)
{
    set_error(std::string(name) + ": bad argument (" + what + ")");
    return RT_ERR_ARG;
}

// probe grids' rules for the struct (api_shade_probes.hip's grid_error, which stays as it is) and flags == 0.
const char* depth_grid_error(const rt_probe_grid* G)
{
    if (!G) return "null grid";
    for (int a = 0; a < 3; a++) {
        if (!pg_finite(G->origin[a])) return "origin not finite";
        if (!pg_finite(G->step[a]) || !(G->step[a] > 0.0)) return "step not finite and above 0";
        if (G->dims[a] < 1) return "dims below 1";
    }
    if ((uint64_t)G->dims[0] * (uint64_t)G->dims[1] >= (1ull << 31) ||
        (uint64_t)G->dims[0] * (uint64_t)G->dims[1] * (uint64_t)G->dims[2] >= (1ull << 31))
        return "2^31 probes or more";
    if (!pg_finite(G->bias) || !(G->bias >= 0.0)) return "bias not finite and at least 0";
    if (G->flags) return "grid flags not 0 (the depth maps are the visibility: no RT_PROBE_GRID_VISIBILITY here)";
    if (G->reserved[0] || G->reserved[1]) return "reserved not 0";
    return nullptr;
}

// The checks of both shading entries; RT_OK with *empty set for n == 0.
int check_shade(const char* name, const rt_probe_grid* G, const rt_probe_depth_params* P, int64_t n, bool null_pointer, bool* empty)
{
    *empty = false;
    const char* bad = depth_grid_error(G);
    if (!bad && !P) bad = "null params";
    if (!bad && !depth_params_ok(P)) bad = kDepthParamsRule;
    if (!bad && n < 0) bad = "n < 0";
    if (bad) return bad_argument(name, bad);
    if (n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (null_pointer) return bad_argument(name, "null pointer");
    return RT_OK;
}

int check_close(const char* name, const void* depth, int64_t n, const void* D, bool* empty)
{
    *empty = n == 0;
    if (n < 0 || n >= (int64_t)1 << 25 || (n > 0 && (!depth || !D))) return bad_argument(name, "null pointer, n < 0 or n >= 2^25");
    return RT_OK;
}

// Samples of one chunk: kQueryChunk (RTCORE_QUERY_CHUNK), as every chunked query entry.
int64_t chunk_samples()
{
    int64_t chunk = kQueryChunk;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(kQueryChunk, atoll(e)));
    return chunk;
}

void fold_probe(const rt_probe_depth_params& P, const rt_ray* rays, const rt_hit* hits, int32_t spp, rt_probe_depth& acc, uint32_t* counts)
{
    double T[kDepthTexels][3];
    for (int t = 0; t < kDepthTexels; t++) oct_texel_dir(t, T[t][0], T[t][1], T[t][2]);
    for (int32_t k = 0; k < spp; k++) {
        const rt_vec4d& d = rays[k].direction;
        if (d.x == 0.0 && d.y == 0.0 && d.z == 0.0) {
            counts[3]++;
            continue;
        }
        const bool hit = hits[k].prim_id >= 0;
        if (hit) {
            counts[0]++;
            if (hits[k].inside != 0) counts[1]++;
        } else {
            counts[2]++;
        }
        const double dist = depth_of(hit, hits[k].distance, P.d_max);
        for (int t = 0; t < kDepthTexels; t++)
            depth_add(T[t][0], T[t][1], T[t][2], d.x, d.y, d.z, dist, P.sharpness, acc.s[0][t], acc.s[1][t], acc.s[2][t]);
    }
}

} // namespace

extern "C" {

int rt_render_probe_depth_device(rt_scene* s, const rt_surfel* d_probes, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                                 uint64_t stream_base, const rt_probe_depth_params* params, rt_probe_depth* d_depth,
                                 uint32_t* d_counts, void* stream)
{
    const char* name = "rt_render_probe_depth_device";
    const char* bad = !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) return RT_OK;
    if (!bad && (!d_probes || !params || !d_depth || !d_counts)) bad = "null pointer";
    if (!bad && !depth_params_ok(params)) bad = kDepthParamsRule;
    if (!bad && spp > kDepthMaxSpp) bad = "spp above 2^19: split the call by sample_base";
    if (bad) return bad_argument(name, bad);
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": runs rt_query_rays' RT_QUERY_FAST kernels (traversal modes BRUTE, GROUPED and BVH); this "
                                      "scene is in BVH2 mode (rt_scene_set_traversal), use RT_TRAVERSAL_BVH");
        return RT_ERR_STATE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t probes = std::min<int64_t>(n, std::max<int64_t>(1, chunk_samples() / spp)); // a chunk holds whole probes
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->probe_depth_rays.reserve((size_t)probes * (size_t)spp));
    HIP_TRY(s->probe_depth_hits.reserve((size_t)probes * (size_t)spp));
    // the rays, their hits, the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    for (int64_t a = 0; a < n; a += probes) {
        const unsigned m = (unsigned)std::min(probes, n - a);
        const unsigned total = m * (unsigned)spp; // (at most 2^19)
        int rc = launch_surfel_rays(RT_GATHER_SPHERE, d_probes + a, total, (unsigned)spp, seed, sample_base, stream_base + (uint64_t)a,
                                    s->probe_depth_rays.p, st);
        if (rc != RT_OK) return rc;
        rc = launch_rays(s, RT_QUERY_FAST, s->probe_depth_rays.p, total, s->probe_depth_hits.p, st);
        if (rc != RT_OK) return rc;
        hipLaunchKernelGGL(probe_depth_fold_kernel, dim3((m + kFoldWaves - 1) / kFoldWaves), dim3(64 * kFoldWaves), 0, st,
                           s->probe_depth_rays.p, s->probe_depth_hits.p, m, (unsigned)spp, params->d_max, params->sharpness, d_depth + a,
                           d_counts + a * 4);
        HIP_TRY(hipGetLastError());
    }
    return end_op(s, st);
}

int rt_debug_probe_depth_fold(const rt_probe_depth_params* params, const rt_ray* rays, const rt_hit* hits, int64_t n, int32_t spp,
                              rt_probe_depth* depth, uint32_t* counts)
{
    const char* name = "rt_debug_probe_depth_fold";
    const char* bad = n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) return RT_OK;
    if (!bad && (!rays || !hits || !params || !depth || !counts)) bad = "null pointer";
    if (!bad && !depth_params_ok(params)) bad = kDepthParamsRule;
    if (bad) return bad_argument(name, bad);
    for (int64_t i = 0; i < n; i++) fold_probe(*params, rays + i * spp, hits + i * spp, spp, depth[i], counts + i * 4);
    return RT_OK;
}

int rt_probe_depth_close_device(const rt_probe_depth* d_depth, int64_t n, double* d_D, void* stream)
{
    bool empty;
    const int rc = check_close("rt_probe_depth_close_device", d_depth, n, d_D, &empty);
    if (rc != RT_OK || empty) return rc;
    const unsigned n_texels = (unsigned)n * (unsigned)kDepthTexels; // (below 2^31)
    hipLaunchKernelGGL(probe_depth_close_kernel, dim3((n_texels + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), d_depth,
                       n_texels, reinterpret_cast<double2*>(d_D));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_debug_probe_depth_close(const rt_probe_depth* depth, int64_t n, double* D)
{
    bool empty;
    const int rc = check_close("rt_debug_probe_depth_close", depth, n, D, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++)
        for (int t = 0; t < kDepthTexels; t++)
            depth_close(depth[i].s[0][t], depth[i].s[1][t], depth[i].s[2][t], D[(i * kDepthTexels + t) * 2], D[(i * kDepthTexels + t) * 2 + 1]);
    return RT_OK;
}

int rt_shade_probes_depth_device(const rt_probe_grid* grid, const rt_probe_depth_params* params, const double* d_L, const double* d_D,
                                 const rt_surfel* d_points, int64_t n, rt_color* d_irradiance, double* d_weight, void* stream)
{
    bool empty;
    const int rc = check_shade("rt_shade_probes_depth_device", grid, params, n, !d_L || !d_D || !d_points || !d_irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t a = 0; a < n; a += kQueryLaunchMax) {
        const unsigned m = (unsigned)std::min(kQueryLaunchMax, n - a);
        hipLaunchKernelGGL(probe_depth_shade_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, *grid, *params, d_L, d_D, d_points + a, m,
                           d_irradiance + a, d_weight ? d_weight + a : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int rt_debug_shade_probes_depth(const rt_probe_grid* grid, const rt_probe_depth_params* params, const double* L, const double* D,
                                const rt_surfel* points, int64_t n, rt_color* irradiance, double* weight)
{
    bool empty;
    const int rc = check_shade("rt_debug_shade_probes_depth", grid, params, n, !L || !D || !points || !irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        double E[3], W;
        depth_blend(*grid, *params, L, D, points[i], c, E, W);
        irradiance[i] = rt_color{E[0], E[1], E[2]};
        if (weight) weight[i] = W;
    }
    return RT_OK;
}

int rt_debug_oct_texel_dirs(double* dirs_out)
{
    if (!dirs_out) return bad_argument("rt_debug_oct_texel_dirs", "null pointer");
    for (int t = 0; t < kDepthTexels; t++) oct_texel_dir(t, dirs_out[3 * t], dirs_out[3 * t + 1], dirs_out[3 * t + 2]);
    return RT_OK;
}

int rt_debug_oct_texel(const double* v, int64_t n, int32_t* texels_out)
{
    if (n < 0 || (n > 0 && (!v || !texels_out))) return bad_argument("rt_debug_oct_texel", "null pointer or n < 0");
    for (int64_t i = 0; i < n; i++) {
        const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
        const bool ok = pg_finite(x) && pg_finite(y) && pg_finite(z) && (x != 0.0 || y != 0.0 || z != 0.0);
        texels_out[i] = ok ? oct_texel(x, y, z) : -1;
    }
    return RT_OK;
}

} // extern "C"
