// api_probe_relocate.hip -- the C ABI's probe relocation (include/rtcore.h, "probe relocation"): per-probe
// offsets and states for a probe grid, the step that derives them from the hit distances of a probe's own
// sample directions, and the shading entries that honour them.  Five kernels (positions, fold, placed
// segments, placed blend, placed depth shade) and their host twins, all compilations of rt_probe_relocate.h.
// A step's chunk is the positions kernel into the scene's scratch, rt_debug_surfel_rays_device's launch
// (launch_surfel_rays) and rt_query_rays_device's closest-hit launch (launch_rays) as the depth bake runs them
// (api_probe_depth.hip), and the fold.  The unplaced kernels of api_shade_probes.hip and api_probe_depth.hip
// are not touched: the placed ones are kernels of their own.
#include <cstdlib>
#include <cstring>

#include "rt_probe_relocate.h"
#include "rt_scene.h"

static_assert(sizeof(rt_probe_relocate_params) == 32, "rt_probe_relocate_params: two 16-byte rows");
static_assert(sizeof(rt_probe_relocation) == 64, "rt_probe_relocation: four 16-byte rows");
static_assert(sizeof(rt_hit) == 48 && sizeof(rt_ray) == 64, "the step's scratch: 64 + 48 B per sample");

namespace {

constexpr int32_t kRelocateMaxSpp = 1 << 19; // one probe's samples are one chunk at the most
constexpr int kFoldWaves = 4;                // probes per block of the fold kernel

// One thread per probe of [first, first + m).
__global__ void __launch_bounds__(256) probe_positions_kernel(rt_probe_grid G, const double* __restrict__ offsets, unsigned first, unsigned m,
                                                              rt_surfel* __restrict__ out)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    out[j] = placed_surfel(G, offsets, (int64_t)first + j);
}

// One wave per probe.  Lane l folds the samples k = l, l + 64, ... in ascending order with the definition's
// strict comparisons, so it holds the lowest k of its best distance; the 64 lanes' (d, k) pairs are then
// reduced by six __shfl_xor steps under reloc_less / reloc_more, a total order on the pairs that can win, so
// every lane ends with the same winners and they are the sequential fold's whatever the lane layout.  The
// counts are integer sums.  The winners' sample numbers are made wave-uniform (readfirstlane) and lane 0
// re-reads their directions, applies the rule and stores.
__global__ void __launch_bounds__(64 * kFoldWaves) probe_relocate_fold_kernel(const rt_ray* __restrict__ rays, const rt_hit* __restrict__ hits,
                                                                              unsigned n, unsigned spp, rt_probe_grid G,
                                                                              rt_probe_relocate_params P, double* __restrict__ offsets,
                                                                              rt_probe_relocation* __restrict__ info)
{
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned i = blockIdx.x * (unsigned)kFoldWaves + wave;
    if (i >= n) return;
    const unsigned lane = threadIdx.x & 63u;
    const rt_ray* __restrict__ r = rays + (size_t)i * spp;
    const rt_hit* __restrict__ h = hits + (size_t)i * spp;
    RelocFold f = reloc_fold_start();
    for (unsigned k = lane; k < spp; k += 64u)
        reloc_fold_sample(f, (int32_t)k, r[k].direction.x, r[k].direction.y, r[k].direction.z, h[k].prim_id, h[k].inside, h[k].distance);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        f.front += __shfl_xor(f.front, s);
        f.back += __shfl_xor(f.back, s);
        f.misses += __shfl_xor(f.misses, s);
        f.skipped += __shfl_xor(f.skipped, s);
        double d = __shfl_xor(f.d_near, s);
        int32_t k = __shfl_xor(f.k_near, s);
        if (reloc_less(d, k, f.d_near, f.k_near)) {
            f.d_near = d;
            f.k_near = k;
        }
        d = __shfl_xor(f.d_back, s);
        k = __shfl_xor(f.k_back, s);
        if (reloc_less(d, k, f.d_back, f.k_back)) {
            f.d_back = d;
            f.k_back = k;
        }
        d = __shfl_xor(f.d_far, s);
        k = __shfl_xor(f.k_far, s);
        if (reloc_more(d, k, f.d_far, f.k_far)) {
            f.d_far = d;
            f.k_far = k;
        }
    }
    const int32_t kn = __builtin_amdgcn_readfirstlane(f.k_near), kb = __builtin_amdgcn_readfirstlane(f.k_back),
                  kf = __builtin_amdgcn_readfirstlane(f.k_far);
    if (lane != 0u) return;
    double Dn[3] = {0.0, 0.0, 0.0}, Db[3] = {0.0, 0.0, 0.0}, Df[3] = {0.0, 0.0, 0.0};
    if (kn >= 0) Dn[0] = r[kn].direction.x, Dn[1] = r[kn].direction.y, Dn[2] = r[kn].direction.z;
    if (kb >= 0) Db[0] = r[kb].direction.x, Db[1] = r[kb].direction.y, Db[2] = r[kb].direction.z;
    if (kf >= 0) Df[0] = r[kf].direction.x, Df[1] = r[kf].direction.y, Df[2] = r[kf].direction.z;
    double* o = offsets + (size_t)i * 3;
    const double was[3] = {o[0], o[1], o[2]};
    double c[3];
    info[i] = reloc_rule(G, P, f, (int32_t)spp, was, Db, Dn, Df, c);
    if (!(P.flags & RT_PROBE_RELOCATE_CLASSIFY_ONLY)) {
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
    }
}

// probe_segments_kernel (api_shade_probes.hip) over placed probes.
__global__ void __launch_bounds__(256) probe_segments_placed_kernel(rt_probe_grid G, const double* __restrict__ offsets,
                                                                    const uint32_t* __restrict__ state, const rt_surfel* __restrict__ points,
                                                                    unsigned n_seg, rt_ray* __restrict__ rays, double* __restrict__ t_max)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_seg) return;
    const rt_surfel s = points[j >> 3];
    const ProbeCell c = probe_cell(G, s);
    const int k = (int)(j & 7u);
    double t = c.t[0];
#pragma unroll
    for (int q = 1; q < kProbeCorners; q++) t = k == q ? c.t[q] : t;
    rt_ray r;
    double tm;
    placed_segment_at(G, offsets, state, s, c, k, t, r, tm);
    rays[j] = r;
    t_max[j] = tm;
}

// probe_blend_kernel over placed probes: the absent corners join the hidden ones.
__global__ void __launch_bounds__(256) probe_blend_placed_kernel(rt_probe_grid G, const double* __restrict__ offsets,
                                                                 const uint32_t* __restrict__ state, const double* __restrict__ L,
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
    probe_blend(G, L, c, hidden | placed_absent(G, offsets, state, c), E, W);
    irradiance[i] = rt_color{E[0], E[1], E[2]};
    if (weight) weight[i] = W;
}

// probe_depth_shade_kernel (api_probe_depth.hip) over placed probes.  Two waves per SIMD at the most, as that
// kernel comes out at: left to itself the compiler aims at three here and spills 120 B per lane for it.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) probe_depth_shade_placed_kernel(rt_probe_grid G, const double* __restrict__ offsets,
                                                                       const uint32_t* __restrict__ state, rt_probe_depth_params P,
                                                                       const double* __restrict__ L, const double* __restrict__ D,
                                                                       const rt_surfel* __restrict__ points, unsigned n,
                                                                       rt_color* __restrict__ irradiance, double* __restrict__ weight)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rt_surfel s = points[i];
    const ProbeCell c = probe_cell(G, s);
    double E[3], W;
    placed_depth_blend(G, offsets, state, P, L, D, s, c, E, W);
    irradiance[i] = rt_color{E[0], E[1], E[2]};
    if (weight) weight[i] = W;
}

int bad_argument(const char* name, const char* what)
{
    set_error(std::string(name) + ": bad argument (" + what + ")");
    return RT_ERR_ARG;
}

// probe grids' rules for the struct; `flags`: the flag bits the entry accepts.
const char* placed_grid_error(const rt_probe_grid* G, uint32_t flags)
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
    if (G->flags & ~flags) return flags ? "unknown flag bits" : "grid flags not 0 (the depth maps are the visibility: no RT_PROBE_GRID_VISIBILITY here)";
    if (G->reserved[0] || G->reserved[1]) return "reserved not 0";
    return nullptr;
}

int64_t grid_probes(const rt_probe_grid& G) { return (int64_t)G.dims[0] * G.dims[1] * G.dims[2]; }

// The argument checks of the entries over a grid and n points; RT_OK with *empty set for n == 0.
int check_points(const char* name, bool scene_missing, const rt_probe_grid* G, uint32_t flags, bool params_bad, int64_t n, bool null_pointer,
                 bool* empty)
{
    *empty = false;
    const char* bad = scene_missing ? "null scene" : placed_grid_error(G, flags);
    if (!bad && params_bad) bad = kDepthParamsRule;
    if (!bad && n < 0) bad = "n < 0";
    if (bad) return bad_argument(name, bad);
    if (n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (null_pointer) return bad_argument(name, "null pointer");
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

// Samples of one chunk: kQueryChunk (RTCORE_QUERY_CHUNK), as every chunked query entry.
int64_t chunk_samples()
{
    int64_t chunk = kQueryChunk;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(kQueryChunk, atoll(e)));
    return chunk;
}
int64_t chunk_points() { return std::max<int64_t>(1, chunk_samples() / kProbeCorners); }

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// rt_shade_probes_placed_device after its checks and the stream ordering, as api_shade_probes.hip's shade_chunks.
int shade_chunks(rt_scene* s, const rt_probe_grid& G, const double* d_offsets, const uint32_t* d_state, const double* d_L,
                 const rt_surfel* d_points, int64_t n, rt_color* d_irradiance, double* d_weight, hipStream_t st)
{
    const bool vis = (G.flags & RT_PROBE_GRID_VISIBILITY) != 0;
    const int64_t chunk = vis ? chunk_points() : kQueryLaunchMax;
    for (int64_t a = 0; a < n; a += chunk) {
        const unsigned m = (unsigned)std::min(chunk, n - a);
        if (vis) {
            const unsigned n_seg = m * (unsigned)kProbeCorners;
            hipLaunchKernelGGL(probe_segments_placed_kernel, dim3(blocks_of(n_seg)), dim3(256), 0, st, G, d_offsets, d_state, d_points + a,
                               n_seg, s->probe_seg_rays.p, s->probe_seg_t_max.p);
            HIP_TRY(hipGetLastError());
            const int rc = launch_segments(s, RT_QUERY_FAST, s->probe_seg_rays.p, s->probe_seg_t_max.p, n_seg, s->probe_seg_occluded.p, st);
            if (rc != RT_OK) return rc;
        }
        hipLaunchKernelGGL(probe_blend_placed_kernel, dim3(blocks_of(m)), dim3(256), 0, st, G, d_offsets, d_state, d_L, d_points + a,
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

// The host fold of one probe and the rule.
void relocate_probe(const rt_probe_grid& G, const rt_probe_relocate_params& P, const rt_ray* rays, const rt_hit* hits, int32_t spp,
                    double* o, rt_probe_relocation& info)
{
    RelocFold f = reloc_fold_start();
    for (int32_t k = 0; k < spp; k++)
        reloc_fold_sample(f, k, rays[k].direction.x, rays[k].direction.y, rays[k].direction.z, hits[k].prim_id, hits[k].inside,
                          hits[k].distance);
    double D[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const int32_t ks[3] = {f.k_back, f.k_near, f.k_far};
    for (int j = 0; j < 3; j++)
        if (ks[j] >= 0) D[j][0] = rays[ks[j]].direction.x, D[j][1] = rays[ks[j]].direction.y, D[j][2] = rays[ks[j]].direction.z;
    const double was[3] = {o[0], o[1], o[2]};
    double c[3];
    info = reloc_rule(G, P, f, spp, was, D[0], D[1], D[2], c);
    if (!(P.flags & RT_PROBE_RELOCATE_CLASSIFY_ONLY))
        for (int a = 0; a < 3; a++) o[a] = c[a];
}

const char* relocate_error(bool scene_missing, const rt_probe_grid* G, const rt_probe_relocate_params* P, int32_t spp, bool null_pointer)
{
    const char* bad = scene_missing ? "null scene" : placed_grid_error(G, RT_PROBE_GRID_VISIBILITY);
    if (!bad && !P) bad = "null params";
    if (!bad && !relocate_params_ok(P)) bad = kRelocateParamsRule;
    if (!bad && spp <= 0) bad = "spp <= 0";
    if (!bad && spp > kRelocateMaxSpp) bad = "spp above 2^19: take several steps";
    if (!bad && null_pointer) bad = "null pointer";
    return bad;
}

} // namespace

extern "C" {

int rt_probe_positions_device(const rt_probe_grid* grid, const double* d_offsets, rt_surfel* d_probes_out, void* stream)
{
    const char* name = "rt_probe_positions_device";
    const char* bad = placed_grid_error(grid, RT_PROBE_GRID_VISIBILITY);
    if (!bad && !d_probes_out) bad = "null pointer";
    if (bad) return bad_argument(name, bad);
    const unsigned n = (unsigned)grid_probes(*grid); // (below 2^31)
    hipLaunchKernelGGL(probe_positions_kernel, dim3(blocks_of(n)), dim3(256), 0, static_cast<hipStream_t>(stream), *grid, d_offsets, 0u, n,
                       d_probes_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_debug_probe_positions(const rt_probe_grid* grid, const double* offsets, rt_surfel* probes_out)
{
    const char* bad = placed_grid_error(grid, RT_PROBE_GRID_VISIBILITY);
    if (!bad && !probes_out) bad = "null pointer";
    if (bad) return bad_argument("rt_debug_probe_positions", bad);
    const int64_t n = grid_probes(*grid);
    for (int64_t p = 0; p < n; p++) probes_out[p] = placed_surfel(*grid, offsets, p);
    return RT_OK;
}

int rt_relocate_probes_device(rt_scene* s, const rt_probe_grid* grid, const rt_probe_relocate_params* params, int32_t spp, uint64_t seed,
                              uint64_t sample_base, uint64_t stream_base, double* d_offsets, rt_probe_relocation* d_info, void* stream)
{
    const char* name = "rt_relocate_probes_device";
    if (const char* bad = relocate_error(!s, grid, params, spp, !d_offsets || !d_info)) return bad_argument(name, bad);
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": runs rt_query_rays' RT_QUERY_FAST kernels (traversal modes BRUTE, GROUPED and BVH); this "
                                      "scene is in BVH2 mode (rt_scene_set_traversal), use RT_TRAVERSAL_BVH");
        return RT_ERR_STATE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n = grid_probes(*grid);
    const int64_t probes = std::min<int64_t>(n, std::max<int64_t>(1, chunk_samples() / spp)); // a chunk holds whole probes
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->probe_depth_rays.reserve((size_t)probes * (size_t)spp));
    HIP_TRY(s->probe_depth_hits.reserve((size_t)probes * (size_t)spp));
    HIP_TRY(s->shade_points.reserve((size_t)probes));
    // the positions, the rays, their hits, the work counter and the stack overflow area are the scene's: order
    // after its last operation
    HIP_TRY(wait_last_op(s, st));
    for (int64_t a = 0; a < n; a += probes) {
        const unsigned m = (unsigned)std::min(probes, n - a);
        const unsigned total = m * (unsigned)spp; // (at most 2^19)
        hipLaunchKernelGGL(probe_positions_kernel, dim3(blocks_of(m)), dim3(256), 0, st, *grid, d_offsets, (unsigned)a, m, s->shade_points.p);
        HIP_TRY(hipGetLastError());
        int rc = launch_surfel_rays(RT_GATHER_SPHERE, s->shade_points.p, total, (unsigned)spp, seed, sample_base, stream_base + (uint64_t)a,
                                    s->probe_depth_rays.p, st);
        if (rc != RT_OK) return rc;
        rc = launch_rays(s, RT_QUERY_FAST, s->probe_depth_rays.p, total, s->probe_depth_hits.p, st);
        if (rc != RT_OK) return rc;
        hipLaunchKernelGGL(probe_relocate_fold_kernel, dim3((m + kFoldWaves - 1) / kFoldWaves), dim3(64 * kFoldWaves), 0, st,
                           s->probe_depth_rays.p, s->probe_depth_hits.p, m, (unsigned)spp, *grid, *params, d_offsets + a * 3, d_info + a);
        HIP_TRY(hipGetLastError());
    }
    return end_op(s, st);
}

int rt_debug_probe_relocate(const rt_probe_grid* grid, const rt_probe_relocate_params* params, const rt_ray* rays, const rt_hit* hits,
                            int32_t spp, double* offsets, rt_probe_relocation* info)
{
    if (const char* bad = relocate_error(false, grid, params, spp, !rays || !hits || !offsets || !info))
        return bad_argument("rt_debug_probe_relocate", bad);
    const int64_t n = grid_probes(*grid);
    for (int64_t i = 0; i < n; i++) relocate_probe(*grid, *params, rays + i * spp, hits + i * spp, spp, offsets + i * 3, info[i]);
    return RT_OK;
}

int rt_shade_probes_placed_device(rt_scene* s, const rt_probe_grid* grid, const double* d_offsets, const uint32_t* d_state, const double* d_L,
                                  const rt_surfel* d_points, int64_t n, rt_color* d_irradiance, double* d_weight, void* stream)
{
    const char* name = "rt_shade_probes_placed_device";
    bool empty;
    int rc = check_points(name, !s, grid, RT_PROBE_GRID_VISIBILITY, false, n, !d_L || !d_points || !d_irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    rc = check_state(name, s, grid);
    if (rc != RT_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(s->device));
    rc = reserve_segments(s, *grid, n);
    if (rc != RT_OK) return rc;
    HIP_TRY(wait_last_op(s, st));
    rc = shade_chunks(s, *grid, d_offsets, d_state, d_L, d_points, n, d_irradiance, d_weight, st);
    if (rc != RT_OK) return rc;
    return end_op(s, st);
}

// rt_shade_probes' chunks; the offsets and the states go up once, behind L in its buffer.
int rt_shade_probes_placed(rt_scene* s, const rt_probe_grid* grid, const double* offsets, const uint32_t* state, const double* L,
                           const rt_surfel* points, int64_t n, rt_color* irradiance, double* weight)
{
    const char* name = "rt_shade_probes_placed";
    bool empty;
    int rc = check_points(name, !s, grid, RT_PROBE_GRID_VISIBILITY, false, n, !L || !points || !irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    rc = check_state(name, s, grid);
    if (rc != RT_OK) return rc;
    const size_t n_probes = (size_t)grid_probes(*grid), n_L = n_probes * kProbeL;
    const size_t n_state = (n_probes + 1) / 2; // doubles that hold n_probes uint32
    const int64_t chunk = std::min(chunk_points(), n);
    hipStream_t st = s->stream;
    HIP_TRY(hipSetDevice(s->device));
    rc = reserve_segments(s, *grid, n);
    if (rc != RT_OK) return rc;
    HIP_TRY(s->shade_L.reserve(n_L + n_probes * 3 + n_state));
    HIP_TRY(s->shade_points.reserve((size_t)chunk));
    HIP_TRY(s->shade_out.reserve((size_t)chunk * 4));
    HIP_TRY(wait_last_op(s, st));
    double* d_offsets = offsets ? s->shade_L.p + n_L : nullptr;
    uint32_t* d_state = state ? reinterpret_cast<uint32_t*>(s->shade_L.p + n_L + n_probes * 3) : nullptr;
    HIP_TRY(hipMemcpyAsync(s->shade_L.p, L, n_L * sizeof(double), hipMemcpyHostToDevice, st));
    if (offsets) HIP_TRY(hipMemcpyAsync(d_offsets, offsets, n_probes * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (state) HIP_TRY(hipMemcpyAsync(d_state, state, n_probes * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rt_color* d_irr = reinterpret_cast<rt_color*>(s->shade_out.p);
    double* d_w = s->shade_out.p + (size_t)chunk * 3;
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        HIP_TRY(hipMemcpyAsync(s->shade_points.p, points + a, (size_t)m * sizeof(rt_surfel), hipMemcpyHostToDevice, st));
        rc = shade_chunks(s, *grid, d_offsets, d_state, s->shade_L.p, s->shade_points.p, m, d_irr, d_w, st);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(irradiance + a, d_irr, (size_t)m * sizeof(rt_color), hipMemcpyDeviceToHost, st));
        if (weight) HIP_TRY(hipMemcpyAsync(weight + a, d_w, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return end_op(s, st);
}

int rt_debug_probe_segments_placed_device(const rt_probe_grid* grid, const double* d_offsets, const uint32_t* d_state,
                                          const rt_surfel* d_points, int64_t n, rt_ray* d_rays_out, double* d_t_max_out, void* stream)
{
    bool empty;
    const int rc = check_points("rt_debug_probe_segments_placed_device", false, grid, RT_PROBE_GRID_VISIBILITY, false, n,
                                !d_points || !d_rays_out || !d_t_max_out, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t most = (int64_t)1 << 28; // points of one launch (32-bit segment indices)
    for (int64_t a = 0; a < n; a += most) {
        const unsigned n_seg = (unsigned)(std::min(most, n - a) * kProbeCorners);
        hipLaunchKernelGGL(probe_segments_placed_kernel, dim3(blocks_of(n_seg)), dim3(256), 0, st, *grid, d_offsets, d_state, d_points + a,
                           n_seg, d_rays_out + a * kProbeCorners, d_t_max_out + a * kProbeCorners);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int rt_debug_probe_segments_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state, const rt_surfel* points,
                                   int64_t n, rt_ray* rays_out, double* t_max_out)
{
    bool empty;
    const int rc = check_points("rt_debug_probe_segments_placed", false, grid, RT_PROBE_GRID_VISIBILITY, false, n,
                                !points || !rays_out || !t_max_out, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        for (int k = 0; k < kProbeCorners; k++)
            placed_segment_at(*grid, offsets, state, points[i], c, k, c.t[k], rays_out[i * kProbeCorners + k], t_max_out[i * kProbeCorners + k]);
    }
    return RT_OK;
}

int rt_debug_shade_probes_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state, const double* L,
                                 const rt_surfel* points, int64_t n, const uint8_t* occluded, rt_color* irradiance, double* weight)
{
    bool empty;
    const int rc = check_points("rt_debug_shade_probes_placed", false, grid, RT_PROBE_GRID_VISIBILITY, false, n, !L || !points || !irradiance,
                                &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        double E[3], W;
        probe_blend(*grid, L, c, probe_hidden(occluded ? occluded + i * kProbeCorners : nullptr) | placed_absent(*grid, offsets, state, c), E,
                    W);
        irradiance[i] = rt_color{E[0], E[1], E[2]};
        if (weight) weight[i] = W;
    }
    return RT_OK;
}

int rt_shade_probes_depth_placed_device(const rt_probe_grid* grid, const double* d_offsets, const uint32_t* d_state,
                                        const rt_probe_depth_params* params, const double* d_L, const double* d_D, const rt_surfel* d_points,
                                        int64_t n, rt_color* d_irradiance, double* d_weight, void* stream)
{
    const char* name = "rt_shade_probes_depth_placed_device";
    if (grid && !placed_grid_error(grid, 0u) && !params) return bad_argument(name, "null params");
    bool empty;
    const int rc = check_points(name, false, grid, 0u, !depth_params_ok(params), n, !d_L || !d_D || !d_points || !d_irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t a = 0; a < n; a += kQueryLaunchMax) {
        const unsigned m = (unsigned)std::min(kQueryLaunchMax, n - a);
        hipLaunchKernelGGL(probe_depth_shade_placed_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, *grid, d_offsets, d_state, *params, d_L,
                           d_D, d_points + a, m, d_irradiance + a, d_weight ? d_weight + a : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

int rt_debug_shade_probes_depth_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state,
                                       const rt_probe_depth_params* params, const double* L, const double* D, const rt_surfel* points,
                                       int64_t n, rt_color* irradiance, double* weight)
{
    const char* name = "rt_debug_shade_probes_depth_placed";
    if (grid && !placed_grid_error(grid, 0u) && !params) return bad_argument(name, "null params");
    bool empty;
    const int rc = check_points(name, false, grid, 0u, !depth_params_ok(params), n, !L || !D || !points || !irradiance, &empty);
    if (rc != RT_OK || empty) return rc;
    for (int64_t i = 0; i < n; i++) {
        const ProbeCell c = probe_cell(*grid, points[i]);
        double E[3], W;
        placed_depth_blend(*grid, offsets, state, *params, L, D, points[i], c, E, W);
        irradiance[i] = rt_color{E[0], E[1], E[2]};
        if (weight) weight[i] = W;
    }
    return RT_OK;
}

} // extern "C"
