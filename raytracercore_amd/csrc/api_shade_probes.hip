// api_shade_probes.hip -- the C ABI's probe grids (include/rtcore.h, "probe grids", rt_probe_grid): the
// radiance coefficients L of rt_render_probes' accumulators, and the irradiance a grid of such probes gives
// at shading points: a trilinear blend over the cell's eight probes, without those the point cannot see, then
// the nine-term dot product with the cosine lobe.  Three kernels (radiance, segments, blend) and their host
// twins, all compilations of rt_probe_grid.h; the visibility is rt_occluded_rays' any-hit launch
// (launch_segments, api_query.hip) over the segments the second kernel writes into the scene's scratch, as
// rt_primary_hits_device runs the closest-hit launch over the camera rays it makes.
#include <cstdlib>
#include <cstring>

#include "rt_probe_grid.h"
#include "rt_scene.h"

static_assert(sizeof(rt_probe_grid) == 80, "rt_probe_grid: five 16-byte rows");

namespace {

// One thread per probe: 296 B read, 216 B written.
__global__ void __launch_bounds__(256) probe_radiance_kernel(const rt_probe_sh* __restrict__ sh, const uint32_t* __restrict__ samples,
                                                             const uint32_t* __restrict__ misses, unsigned n, rt_color ambient,
                                                             double* __restrict__ L)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rt_probe_sh c = sh[i];
    double out[kProbeL];
    probe_radiance(c, samples[i], misses[i], ambient, out);
#pragma unroll
    for (int j = 0; j < kProbeL; j++) L[(size_t)i * kProbeL + j] = out[j];
}

// One thread per (point, corner): lane & 7 is the corner, so a wave's stores are 64 consecutive segments.
// The eight lanes of a point each work out its cell (a few dozen fp64 operations) rather than share it.
__global__ void __launch_bounds__(256) probe_segments_kernel(rt_probe_grid G, const rt_surfel* __restrict__ points, unsigned n_seg,
                                                             rt_ray* __restrict__ rays, double* __restrict__ t_max)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_seg) return;
    const rt_surfel s = points[j >> 3];
    const ProbeCell c = probe_cell(G, s);
    const int k = (int)(j & 7u);
    // (the weight by comparisons, not by a register index)
    double t = c.t[0];
#pragma unroll
    for (int q = 1; q < kProbeCorners; q++) t = k == q ? c.t[q] : t;
    rt_ray r;
    double tm;
    probe_segment_at(G, s, c, k, t, r, tm);
    rays[j] = r;
    t_max[j] = tm;
}

// One thread per point: the 27 sums of a point stay in its registers and the corners are
// visited in the order the definition fixes; neighbouring points read the same probes, so a wave's loads of
// L fall on few cache lines.
__global__ void __launch_bounds__(256) probe_blend_kernel(rt_probe_grid G, const double* __restrict__ L,
                                                          const rt_surfel* __restrict__ points, const uint8_t* __restrict__ occluded,
                                                          unsigned n, rt_color* __restrict__ irradiance, double* __restrict__ weight)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const ProbeCell c = probe_cell(G, points[i]);
    unsigned hidden = 0;
    if (occluded) {
        const uint2 w = *reinterpret_cast<const uint2*>(occluded + (size_t)i * kProbeCorners); // (8-byte aligned: 8 i)
#pragma unroll
        for (int k = 0; k < kProbeCorners; k++) hidden |= (((k < 4 ? w.x : w.y) >> (8 * (k & 3))) & 255u) ? 1u << k : 0u;
    }
    double E[3], W;
    probe_blend(G, L, c, hidden, E, W);
    irradiance[i] = rt_color{E[0], E[1], E[2]};
    if (weight) weight[i] = W;
}

const char* grid_error(const rt_probe_grid* G)
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
    if (G->flags & ~RT_PROBE_GRID_VISIBILITY) return "unknown flag bits";
    if (G->reserved[0] || G->reserved[1]) return "reserved not 0";
    return nullptr;
}

// The argument checks of every entry over a grid and n points; RT_OK with *empty set for n == 0.
int check_grid(const char* name, bool scene_missing, const rt_probe_grid* G, int64_t n, bool null_pointer, bool* empty)
{
    *empty = false;
    const char* bad = scene_missing ? "null scene" : grid_error(G);
    if (!bad && n < 0) bad = "n < 0";
    if (!bad && n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!bad && null_pointer) bad = "null pointer";
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int check_radiance(const char* name, const void* sh, const void* samples, const void* misses, int64_t n, const void* L, bool* empty)
{
    *empty = n == 0;
    if (n < 0 || (n > 0 && (!sh || !samples || !misses || !L))) {
        set_error(std::string(name) + ": bad argument (null pointer or n < 0)");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int check_state(const char* name, const rt_scene* s, const rt_probe_grid* G)
{
    if ((G->flags & RT_PROBE_GRID_VISIBILITY) && s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": RT_PROBE_GRID_VISIBILITY runs rt_occluded_rays' RT_QUERY_FAST kernels (traversal modes "
                                      "BRUTE, GROUPED and BVH); this scene is in BVH2 mode (rt_scene_set_traversal)");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

// Points of one chunk: kQueryChunk / 8 (RTCORE_QUERY_CHUNK / 8), so a chunk's segments are one any-hit launch.
int64_t chunk_points()
{
    int64_t chunk = kQueryChunk;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(kQueryChunk, atoll(e)));
    return std::max<int64_t>(1, chunk / kProbeCorners);
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// rt_shade_probes_device after its checks and the stream ordering: the chunks' launches on `st`.
int shade_chunks(rt_scene* s, const rt_probe_grid& G, const double* d_L, const rt_surfel* d_points, int64_t n, rt_color* d_irradiance,
                 double* d_weight, hipStream_t st)
{
    const bool vis = (G.flags & RT_PROBE_GRID_VISIBILITY) != 0;
    const int64_t chunk = vis ? chunk_points() : kQueryLaunchMax;
    for (int64_t a = 0; a < n; a += chunk) {
        const unsigned m = (unsigned)std::min(chunk, n - a);
        if (vis) {
            const unsigned n_seg = m * (unsigned)kProbeCorners;
            hipLaunchKernelGGL(probe_segments_kernel, dim3(blocks_of(n_seg)), dim3(256), 0, st, G, d_points + a, n_seg,
                               s->probe_seg_rays.p, s->probe_seg_t_max.p);
            HIP_TRY(hipGetLastError());
            const int rc = launch_segments(s, RT_QUERY_FAST, s->probe_seg_rays.p, s->probe_seg_t_max.p, n_seg, s->probe_seg_occluded.p, st);
            if (rc != RT_OK) return rc;
        }
        hipLaunchKernelGGL(probe_blend_kernel, dim3(blocks_of(m)), dim3(256), 0, st, G, d_L, d_points + a,
                           vis ? s->probe_seg_occluded.p : nullptr, m, d_irradiance + a, d_weight ? d_weight + a : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int reserve_segments(rt_scene* s, const rt_probe_grid& G, int64_t n)
{
    if (!(G.flags & RT_PROBE_GRID_VISIBILITY)) return RT_OK;
    const size_t n_seg = (size_t)std::min(chunk_points(), n) * kProbeCorners;
    HIP_TRY(s->probe_seg_rays.reserve(n_seg));
    HIP_TRY(s->probe_seg_t_max.reserve(n_seg));
    HIP_TRY(s->probe_seg_occluded.reserve(n_seg));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_probe_radiance_device(const rt_probe_sh* d_sh, const uint32_t* d_samples, const uint32_t* d_misses, int64_t n,
                             rt_color ambient, double* d_L, void* stream)
{
    bool empty;
    const int rc = check_radiance("rt_probe_radiance_device", d_sh, d_samples, d_misses, n, d_L, &empty);
    if (rc != RT_OK || empty) return rc;
    if (n >= (int64_t)1 << 31) {
        set_error("rt_probe_radiance_device: bad argument (2^31 probes or more)");
        return RT_ERR_ARG;
    }
    hipLaunchKernelGGL(probe_radiance_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, static_cast<hipStream_t>(stream), d_sh,
                       d_samples, d_misses, (unsigned)n, ambient, d_L);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_debug_probe_radiance(const rt_probe_sh* sh, const uint32_t* samples, const uint32_t* misses, int64_t n, rt_color ambient,
                            double* L)
{
    bool empty;
    const int rc = check_radiance("rt_debug_probe_radiance", sh, samples, misses, n, L, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) probe_radiance(sh[i], samples[i], misses[i], ambient, L + i * kProbeL);
    return RT_OK;
}

int rt_shade_probes_device(rt_scene* s, const rt_probe_grid* grid, const double* d_L, const rt_surfel* d_points, int64_t n,
                           rt_color* d_irradiance, double* d_weight, void* stream)
{
    const char* name = "rt_shade_probes_device";
    bool empty;
    int rc = check_grid(name, !s, grid, n, !d_L || !d_points || !d_irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    rc = check_state(name, s, grid);
    if (rc != RT_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    rc = reserve_segments(s, *grid, n);
    if (rc != RT_OK) return rc;
    // the segments, the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    rc = shade_chunks(s, *grid, d_L, d_points, n, d_irradiance, d_weight, st);
    if (rc != RT_OK) return rc;
    return end_op(s, st);
}

// Plain synchronous chunks on the scene's stream: L goes up once, then per chunk the points
// up, the device pass, and the two result arrays down.
int rt_shade_probes(rt_scene* s, const rt_probe_grid* grid, const double* L, const rt_surfel* points, int64_t n,
                    rt_color* irradiance, double* weight)
{
    const char* name = "rt_shade_probes";
    bool empty;
    int rc = check_grid(name, !s, grid, n, !L || !points || !irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    rc = check_state(name, s, grid);
    if (rc != RT_OK) return rc;
    const size_t n_L = (size_t)grid->dims[0] * (size_t)grid->dims[1] * (size_t)grid->dims[2] * kProbeL;
    const int64_t chunk = std::min(chunk_points(), n);
    hipStream_t st = s->stream;
    HIP_TRY(hipSetDevice(s->device));
    rc = reserve_segments(s, *grid, n);
    if (rc != RT_OK) return rc;
    HIP_TRY(s->shade_L.reserve(n_L));
    HIP_TRY(s->shade_points.reserve((size_t)chunk));
    HIP_TRY(s->shade_out.reserve((size_t)chunk * 4));
    HIP_TRY(wait_last_op(s, st));
    HIP_TRY(hipMemcpyAsync(s->shade_L.p, L, n_L * sizeof(double), hipMemcpyHostToDevice, st));
    rt_color* d_irr = reinterpret_cast<rt_color*>(s->shade_out.p);
    double* d_w = s->shade_out.p + (size_t)chunk * 3;
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        HIP_TRY(hipMemcpyAsync(s->shade_points.p, points + a, (size_t)m * sizeof(rt_surfel), hipMemcpyHostToDevice, st));
        rc = shade_chunks(s, *grid, s->shade_L.p, s->shade_points.p, m, d_irr, d_w, st);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(irradiance + a, d_irr, (size_t)m * sizeof(rt_color), hipMemcpyDeviceToHost, st));
        if (weight) HIP_TRY(hipMemcpyAsync(weight + a, d_w, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return end_op(s, st);
}

int rt_debug_probe_segments_device(const rt_probe_grid* grid, const rt_surfel* d_points, int64_t n, rt_ray* d_rays_out,
                                   double* d_t_max_out, void* stream)
{
    bool empty;
    const int rc = check_grid("rt_debug_probe_segments_device", false, grid, n, !d_points || !d_rays_out || !d_t_max_out, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t most = (int64_t)1 << 28; // points of one launch (32-bit segment indices)
    for (int64_t a = 0; a < n; a += most) {
        const unsigned n_seg = (unsigned)(std::min(most, n - a) * kProbeCorners);
        hipLaunchKernelGGL(probe_segments_kernel, dim3(blocks_of(n_seg)), dim3(256), 0, st, *grid, d_points + a, n_seg,
                           d_rays_out + a * kProbeCorners, d_t_max_out + a * kProbeCorners);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int rt_debug_probe_segments(const rt_probe_grid* grid, const rt_surfel* points, int64_t n, rt_ray* rays_out, double* t_max_out)
{
    bool empty;
    const int rc = check_grid("rt_debug_probe_segments", false, grid, n, !points || !rays_out || !t_max_out, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        for (int k = 0; k < kProbeCorners; k++)
            probe_segment_at(*grid, points[i], c, k, c.t[k], rays_out[i * kProbeCorners + k], t_max_out[i * kProbeCorners + k]);
    }
    return RT_OK;
}

int rt_debug_shade_probes(const rt_probe_grid* grid, const double* L, const rt_surfel* points, int64_t n, const uint8_t* occluded,
                          rt_color* irradiance, double* weight)
{
    bool empty;
    const int rc = check_grid("rt_debug_shade_probes", false, grid, n, !L || !points || !irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        double E[3], W;
        probe_blend(*grid, L, c, probe_hidden(occluded ? occluded + i * kProbeCorners : nullptr), E, W);
        irradiance[i] = rt_color{E[0], E[1], E[2]};
        if (weight) weight[i] = W;
    }
    return RT_OK;
}

} // extern "C"
