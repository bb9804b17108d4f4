// api_query.hip -- the C ABI's ray queries (include/rtcore.h, "ray queries"): Scene.RayTrace(ray, null)
// (Scene.cs:113-120) for rays the caller brings, and the camera's own rays on the host; and "occlusion
// queries": whether that query has a hit nearer than a bound, by an any-hit traversal.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "rt_scene.h"

namespace rtc { // (declared in rt_scene.h: api_occluded_surfels.hip launches over the same record)

int query_kernel(const rt_scene* s) { return s->resolved == RT_TRAVERSAL_BVH ? 3 : s->resolved == RT_TRAVERSAL_GROUPED ? 1 : 0; }

int fill_query(rt_scene* s, int kernel, int blocks_per_cu, const rt_ray* d_rays, unsigned n, hipStream_t st, QueryParams& p,
               int& grid)
{
    PathParams h{};
    fill_launch(s->dev, path_variant(kernel, false), h);
    p.rays = reinterpret_cast<const double2*>(d_rays);
    p.n = n;
    p.scene = h.scene;
    p.tests = h.tests;
    p.rows = h.rows;
    p.rects = h.rects;
    p.frames = h.frames;
    p.prims = h.prims;
    p.groups = h.groups;
    p.nodes4 = s->dev.nodes4; // the global nodes, root included: no hot table in this kernel
    p.root4 = s->dev.root4;
    p.n_nodes4 = s->dev.n_nodes4;
    p.xf = h.xf;
    p.vnormals = h.vnormals;
    const int blocks = (int)((n + 255u) / 256u);
    grid = std::min(blocks, s->n_cu * blocks_per_cu);
    if (kernel == 3) {
        HIP_TRY(s->stack_ovf.reserve((size_t)grid * 256 * kStackOverflow));
        HIP_TRY(s->counter.reserve(1));
        HIP_TRY(hipMemsetAsync(s->counter.p, 0, sizeof(unsigned int), st));
        p.counter = s->counter.p;
        p.stack_ovf = s->stack_ovf.p;
        p.spec = 16;
        if (const char* e = getenv("RTCORE_BVH_SPEC")) p.spec = std::max(1, std::min(64, atoi(e)));
    }
    return RT_OK;
}

// rt_occluded_rays: one launch over n <= kQueryLaunchMax segments (d_t_max null: rays).
int launch_segments(rt_scene* s, int32_t mode, const rt_ray* d_rays, const double* d_t_max, unsigned n,
                    unsigned char* d_out, hipStream_t st)
{
    if (mode == RT_QUERY_EXACT) {
        HIP_TRY(launch_occluded_exact(s->dev, d_rays, d_t_max, n, d_out, st));
        return RT_OK;
    }
    const int kernel = query_kernel(s);
    OccludedParams p{};
    int grid = 0;
    const int rc = fill_query(s, kernel, occluded_blocks_per_cu(kernel), d_rays, n, st, p.q, grid);
    if (rc != RT_OK) return rc;
    p.t_max = d_t_max;
    p.out = d_out;
    // the records outside the main loop (planes; BVH: and the outer group) first: measured at or below
    // testing them last in every workload of DESIGN.md 4.5; RTCORE_OCCLUDED_EARLY=0 tests them last (BVH:
    // only for a ray the tree did not answer), for A/B measurements
    p.early = 1;
    if (const char* e = getenv("RTCORE_OCCLUDED_EARLY")) p.early = atoi(e) != 0;
    HIP_TRY(launch_occluded(p, kernel, grid, st));
    return RT_OK;
}

// One launch over n <= kQueryLaunchMax rays on `st`, after the stream ordering is settled.
int launch_rays(rt_scene* s, int32_t mode, const rt_ray* d_rays, unsigned n, rt_hit* d_hits, hipStream_t st)
{
    if (mode == RT_QUERY_EXACT) {
        HIP_TRY(launch_query_exact(s->dev, d_rays, n, d_hits, st));
        return RT_OK;
    }
    const int kernel = query_kernel(s);
    QueryParams p{};
    int grid = 0;
    const int rc = fill_query(s, kernel, query_blocks_per_cu(kernel), d_rays, n, st, p, grid);
    if (rc != RT_OK) return rc;
    p.hits = reinterpret_cast<float4*>(d_hits);
    HIP_TRY(launch_query(p, kernel, grid, st));
    return RT_OK;
}

} // namespace rtc

namespace {

// Argument and state checks shared by both entry points; RT_OK with *empty set for n == 0.
int check_query(rt_scene* s, int32_t mode, const void* rays, int64_t n, const void* hits, const char* name, bool* empty)
{
    *empty = false;
    const bool known_mode = mode == RT_QUERY_FAST || mode == RT_QUERY_EXACT;
    const char* bad = !s ? "null scene" : n < 0 ? "n < 0" : !known_mode ? "unknown mode" : nullptr;
    if (!bad && n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!bad && (!rays || !hits)) bad = "null pointer";
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    if (mode == RT_QUERY_FAST && s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": RT_QUERY_FAST runs in the traversal modes BRUTE, GROUPED and BVH; this scene "
                                      "is in BVH2 mode (rt_scene_set_traversal), use RT_TRAVERSAL_BVH or RT_QUERY_EXACT");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

int query_device(rt_scene* s, int32_t mode, const rt_ray* d_rays, int64_t n, rt_hit* d_hits, hipStream_t st)
{
    if (mode == RT_QUERY_EXACT) {
        const int rc = ensure_ref_bvh(s);
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->device));
    // the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    for (int64_t a = 0; a < n; a += kQueryLaunchMax) {
        const int rc = launch_rays(s, mode, d_rays + a, (unsigned)std::min(kQueryLaunchMax, n - a), d_hits + a, st);
        if (rc != RT_OK) return rc;
    }
    return end_op(s, st);
}

// rt_primary_hits_device's rays: rows [y0, y0 + rows) of the tile's columns [x0, x0 + w), rays[y * w + x],
// by the function rt_camera_rays runs on the host.
__global__ void __launch_bounds__(256) camera_rays_kernel(CameraD cam, int x0, int y0, int w, unsigned n, rt_ray* __restrict__ rays)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int y = (int)(i / (unsigned)w), x = (int)(i - (unsigned)y * (unsigned)w);
    Vec4d o, d;
    camera_ray_d(cam, (double)(x0 + x), (double)(y0 + y), o, d);
    rays[i] = rt_ray{rt_vec4d{o.x, o.y, o.z, o.w}, rt_vec4d{d.x, d.y, d.z, d.w}};
}

} // namespace

extern "C" {

int rt_primary_hits_device(rt_scene* s, int32_t x0, int32_t y0, int32_t w, int32_t h, rt_hit* d_hits, void* stream)
{
    int rc = check_tile(s, x0, y0, w, h);
    if (rc != RT_OK) return rc;
    bool empty;
    rc = check_query(s, RT_QUERY_FAST, d_hits, 1, d_hits, "rt_primary_hits_device", &empty);
    if (rc != RT_OK) return rc;
    if ((int64_t)w > kQueryLaunchMax) {
        set_error("rt_primary_hits_device: bad argument (a row of more than 2^30 pixels)");
        return RT_ERR_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rows =(int)std::min<int64_t>(h, std::max<int64_t>(1, kQueryChunk / w));
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->primary_rays.reserve((size_t)rows * (size_t)w));
    // the rays, the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    for (int r = 0; r < h; r += rows) {
        const unsigned n = (unsigned)std::min(rows, h - r) * (unsigned)w;
        hipLaunchKernelGGL(camera_rays_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, s->camd, x0, y0 + r, w, n,
                           s->primary_rays.p);
        HIP_TRY(hipGetLastError());
        rc = launch_rays(s, RT_QUERY_FAST, s->primary_rays.p, n, d_hits + (size_t)r * (size_t)w, st);
        if (rc != RT_OK) return rc;
    }
    return end_op(s, st);
}

int rt_query_rays_device(rt_scene* s, int32_t mode, const rt_ray* d_rays, int64_t n, rt_hit* d_hits, void* stream)
{
    bool empty;
    const int rc = check_query(s, mode, d_rays, n, d_hits, "rt_query_rays_device", &empty);
    if (rc != RT_OK || empty) return rc;
    return query_device(s, mode, d_rays, n, d_hits, static_cast<hipStream_t>(stream));
}

// The chunk pipeline (run_chunks) with 64 B up and one rt_hit down per ray.
int rt_query_rays(rt_scene* s, int32_t mode, const rt_ray* rays, int64_t n, rt_hit* hits_out)
{
    bool empty;
    int rc = check_query(s, mode, rays, n, hits_out, "rt_query_rays", &empty);
    if (rc != RT_OK || empty) return rc;
    if (mode == RT_QUERY_EXACT) {
        rc = ensure_ref_bvh(s);
        if (rc != RT_OK) return rc;
    }
    rt_ray* stage_rays = nullptr;
    std::atomic<bool> overflow{false};
    ChunkJob job{n, kQueryChunk, 0, sizeof(rt_hit), sizeof(rt_ray), /*one_piece*/ false, /*count_rays*/ false};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C));
        HIP_TRY(s->query_hits.reserve(2 * C));
        stage_rays = reinterpret_cast<rt_ray*>(up);
        d_down = s->query_hits.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        const rt_ray* src = rays + first;
        parallel_ranges(m, 65536,
                        [&](size_t a, size_t b) { std::memcpy(stage_rays + slot + a, src + a, (b - a) * sizeof(rt_ray)); });
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot, stage_rays + slot, m * sizeof(rt_ray), hipMemcpyHostToDevice,
                               s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t, size_t m, size_t slot, hipStream_t st) {
        return launch_rays(s, mode, s->query_rays.p + slot, (unsigned)m, s->query_hits.p + slot, st);
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        const rt_hit* h = reinterpret_cast<const rt_hit*>(stage);
        std::memcpy(hits_out + first + (a - slot), h + a, (b - a) * sizeof(rt_hit));
        if (mode == RT_QUERY_EXACT)
            for (size_t i = a; i < b; i++)
                if (h[i].prim_id == -2) overflow = true;
    };
    rc = run_chunks(s, job);
    if (rc != RT_OK) return rc;
    if (overflow) {
        set_error("rt_query_rays: the reference BVH is deeper than the exact kernel's traversal stack");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

int rt_occluded_rays_device(rt_scene* s, int32_t mode, const rt_ray* d_rays, const double* d_t_max, int64_t n,
                            uint8_t* d_occluded, void* stream)
{
    bool empty;
    int rc = check_query(s, mode, d_rays, n, d_occluded, "rt_occluded_rays_device", &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == RT_QUERY_EXACT) {
        rc = ensure_ref_bvh(s);
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(wait_last_op(s, st));
    for (int64_t a = 0; a < n; a += kQueryLaunchMax) {
        rc = launch_segments(s, mode, d_rays + a, d_t_max ? d_t_max + a : nullptr, (unsigned)std::min(kQueryLaunchMax, n - a),
                             d_occluded + a, st);
        if (rc != RT_OK) return rc;
    }
    return end_op(s, st);
}

// The chunk pipeline (run_chunks) with 72 B up (64 B without t_max) and 1 B down per ray: the rays' two
// staging slots, then the two slots of segment ends.
int rt_occluded_rays(rt_scene* s, int32_t mode, const rt_ray* rays, const double* t_max, int64_t n, uint8_t* occluded_out)
{
    bool empty;
    int rc = check_query(s, mode, rays, n, occluded_out, "rt_occluded_rays", &empty);
    if (rc != RT_OK || empty) return rc;
    if (mode == RT_QUERY_EXACT) {
        rc = ensure_ref_bvh(s);
        if (rc != RT_OK) return rc;
    }
    rt_ray* stage_rays = nullptr;
    double* stage_t = nullptr;
    std::atomic<bool> overflow{false};
    ChunkJob job{n, kQueryChunk, 0, 1, sizeof(rt_ray) + sizeof(double), /*one_piece*/ true, /*count_rays*/ false};
    job.reserve = [&](size_t C, unsigned char* up, const void*& d_down) -> int {
        HIP_TRY(s->query_rays.reserve(2 * C));
        HIP_TRY(s->occluded_out.reserve(2 * C));
        if (t_max) HIP_TRY(s->occluded_t_max.reserve(2 * C));
        stage_rays = reinterpret_cast<rt_ray*>(up);
        stage_t = reinterpret_cast<double*>(stage_rays + 2 * C);
        d_down = s->occluded_out.p;
        return RT_OK;
    };
    job.upload = [&](int64_t, size_t first, size_t m, size_t slot) -> int {
        const rt_ray* src = rays + first;
        const double* src_t = t_max ? t_max + first : nullptr;
        parallel_ranges(m, 65536, [&](size_t a, size_t b) {
            std::memcpy(stage_rays + slot + a, src + a, (b - a) * sizeof(rt_ray));
            if (src_t) std::memcpy(stage_t + slot + a, src_t + a, (b - a) * sizeof(double));
        });
        HIP_TRY(hipMemcpyAsync(s->query_rays.p + slot, stage_rays + slot, m * sizeof(rt_ray), hipMemcpyHostToDevice,
                               s->copy_stream));
        if (src_t)
            HIP_TRY(hipMemcpyAsync(s->occluded_t_max.p + slot, stage_t + slot, m * sizeof(double), hipMemcpyHostToDevice,
                                   s->copy_stream));
        return RT_OK;
    };
    job.launch = [&](int64_t, size_t, size_t m, size_t slot, hipStream_t st) {
        return launch_segments(s, mode, s->query_rays.p + slot, t_max ? s->occluded_t_max.p + slot : nullptr, (unsigned)m,
                               s->occluded_out.p + slot, st);
    };
    job.consume = [&](const unsigned char* stage, size_t a, size_t b, size_t first, size_t slot) {
        std::memcpy(occluded_out + first + (a - slot), stage + a, b - a);
        if (mode == RT_QUERY_EXACT && std::memchr(stage + a, 255, b - a)) overflow = true;
    };
    rc = run_chunks(s, job);
    if (rc != RT_OK) return rc;
    if (overflow) {
        set_error("rt_occluded_rays: the reference BVH is deeper than the exact kernel's traversal stack");
        return RT_ERR_STATE;
    }
    return RT_OK;
}

int rt_camera_rays(const rt_camera* cam, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                   rt_ray* out)
{
    if (!cam || !out || (cam->kind != RT_CAMERA_FRUSTUM && cam->kind != RT_CAMERA_ORTHO) || width <= 0 || height <= 0 ||
        w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || (int64_t)x0 + w > width || (int64_t)y0 + h > height) {
        set_error("rt_camera_rays: bad argument (null pointer, unknown camera kind, w or h <= 0, or a tile outside the frame)");
        return RT_ERR_ARG;
    }
    CameraD camd;
    CameraF camf;
    camera_init(*cam, width, height, camd, camf);
    for (int x = 0; x < w; x++)
        for (int y = 0; y < h; y++) {
            Vec4d o, d;
            camera_ray_d(camd, (double)(x0 + x), (double)(y0 + y), o, d);
            out[(size_t)x * h + y] = rt_ray{rt_vec4d{o.x, o.y, o.z, o.w}, rt_vec4d{d.x, d.y, d.z, d.w}};
        }
    return RT_OK;
}

} // extern "C"
