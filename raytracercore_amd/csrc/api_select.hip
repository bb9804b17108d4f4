// api_select.hip -- the C ABI's selection pass (include/rtcore.h, "selection pass"): DebugRaycaster's
// Selection mode (DebugRaycaster.cs:174-192) for the camera's pixels and for rays the caller brings,
// and its host twin, the same fold (rt_exact_prims.h) compiled for the CPU.
#include <cstring>

#include "rt_exact_prims.h"
#include "rt_scene.h"

namespace {

constexpr int64_t kSelectChunk = 1 << 19;     // rays of one chunk of rt_select_rays
constexpr int64_t kSelectLaunchMax = 1 << 30; // rays of one launch (32-bit ray indices)

int bad_arg(const char* name, const std::string& what)
{
    set_error(std::string(name) + ": bad argument (" + what + ")");
    return RT_ERR_ARG;
}

// The checks of an item list that need no reference BVH: kinds, primitive indices, the test bound.
// *nodes is set when a node item is present (its index is checked once the BVH is there).
int check_items(const char* name, const rt_select_item* items, int32_t n_items, int n_prims, uint64_t n_rays, bool* nodes)
{
    *nodes = false;
    if (n_items > 0 && n_rays > RT_SELECT_MAX_TESTS / (uint64_t)n_items)
        return bad_arg(name, "more than RT_SELECT_MAX_TESTS = 2^32 item tests (rays or pixels x items) in one call; "
                             "split the tile, the rays or the list");
    for (int32_t k = 0; k < n_items; k++) {
        const rt_select_item& it = items[k];
        if (it.kind == RT_SELECT_NODE)
            *nodes = true;
        else if (it.kind != RT_SELECT_PRIM)
            return bad_arg(name, "unknown kind at item " + std::to_string(k));
        else if (it.index < 0 || it.index >= n_prims)
            return bad_arg(name, "primitive index outside [0, n_prims) at item " + std::to_string(k));
    }
    return RT_OK;
}

int check_nodes(const char* name, const rt_select_item* items, int32_t n_items, int n_nodes)
{
    for (int32_t k = 0; k < n_items; k++)
        if (items[k].kind == RT_SELECT_NODE && (items[k].index < 0 || items[k].index >= n_nodes))
            return bad_arg(name, "node index outside the reference BVH at item " + std::to_string(k));
    return RT_OK;
}

// What both device entry points do before their launch: the checks, the reference BVH when a node
// item asks for it, the stream ordering against the scene's previous operation (the item buffer is
// the scene's), and the list's copy to the device on `st`.
int prepare_items(rt_scene* s, const char* name, const rt_select_item* items, int32_t n_items, uint64_t n_rays,
                  hipStream_t st)
{
    bool nodes;
    int rc = check_items(name, items, n_items, (int)s->host.size(), n_rays, &nodes);
    if (rc != RT_OK) return rc;
    if (nodes) {
        rc = ensure_ref_bvh(s);
        if (rc != RT_OK) return rc;
        rc = check_nodes(name, items, n_items, s->dev.n_ref_nodes);
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(s->select_items.reserve((size_t)n_items));
    if (s->any_op && st != s->last_stream) HIP_TRY(hipStreamWaitEvent(st, s->done_ev, 0));
    // from the caller's pageable array: the runtime has taken the bytes when the call returns, and
    // the copy itself is ordered on st behind the previous list's kernel
    if (n_items > 0)
        HIP_TRY(hipMemcpyAsync(s->select_items.p, items, (size_t)n_items * sizeof(rt_select_item), hipMemcpyHostToDevice, st));
    return RT_OK;
}

int check_pixels(rt_scene* s, const char* name, const rt_select_item* items, int32_t n_items, int32_t x0, int32_t y0,
                 int32_t w, int32_t h, const void* out)
{
    if (!s) return bad_arg(name, "null scene");
    if (n_items < 0) return bad_arg(name, "n_items < 0");
    if (!out || (n_items > 0 && !items)) return bad_arg(name, "null pointer");
    const int rc = check_tile(s, x0, y0, w, h);
    if (rc == RT_ERR_ARG) return bad_arg(name, "tile outside the frame");
    return rc;
}

int select_pixels_device(rt_scene* s, const char* name, const rt_select_item* items, int32_t n_items, int32_t x0,
                         int32_t y0, int32_t w, int32_t h, rt_selection* d_out, hipStream_t st)
{
    int rc = prepare_items(s, name, items, n_items, (uint64_t)w * (uint64_t)h, st);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_select_pixels(s->dev, s->camd, s->select_items.p, n_items, x0, y0, w, h, d_out, st));
    return end_op(s, st);
}

// RT_OK with *empty set for n == 0.
int check_rays(rt_scene* s, const char* name, const rt_select_item* items, int32_t n_items, const void* rays, int64_t n,
               const void* out, bool* empty)
{
    *empty = false;
    if (!s) return bad_arg(name, "null scene");
    if (n_items < 0) return bad_arg(name, "n_items < 0");
    if (n < 0) return bad_arg(name, "n < 0");
    if (n == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!rays || !out || (n_items > 0 && !items)) return bad_arg(name, "null pointer");
    return RT_OK;
}

// The launches over n device-resident rays, once prepare_items has run on `st`.
int launch_rays(rt_scene* s, int32_t n_items, const rt_ray* d_rays, int64_t n, rt_selection* d_out, hipStream_t st)
{
    for (int64_t a = 0; a < n; a += kSelectLaunchMax)
        HIP_TRY(launch_select_rays(s->dev, s->select_items.p, n_items, d_rays + a, (unsigned)std::min(kSelectLaunchMax, n - a),
                                   d_out + a, st));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_select_pixels_device(rt_scene* s, const rt_select_item* items, int32_t n_items, int32_t x0, int32_t y0, int32_t w,
                            int32_t h, rt_selection* d_out, void* stream)
{
    const char* name = "rt_select_pixels_device";
    const int rc = check_pixels(s, name, items, n_items, x0, y0, w, h, d_out);
    if (rc != RT_OK) return rc;
    return select_pixels_device(s, name, items, n_items, x0, y0, w, h, d_out, static_cast<hipStream_t>(stream));
}

int rt_select_pixels(rt_scene* s, const rt_select_item* items, int32_t n_items, int32_t x0, int32_t y0, int32_t w,
                     int32_t h, rt_selection* out)
{
    const char* name = "rt_select_pixels";
    int rc = check_pixels(s, name, items, n_items, x0, y0, w, h, out);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t npix = (size_t)w * h;
    HIP_TRY(s->select_out.reserve(npix));
    rc = select_pixels_device(s, name, items, n_items, x0, y0, w, h, s->select_out.p, s->stream);
    if (rc != RT_OK) return rc;
    std::vector<rt_selection> tmp(npix);
    HIP_TRY(hipMemcpyAsync(tmp.data(), s->select_out.p, npix * sizeof(rt_selection), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    parallel_ranges((size_t)w, 64, [&](size_t xa, size_t xb) { // column ranges: disjoint output spans
        for (int y = 0; y < h; y++)
            for (size_t x = xa; x < xb; x++) out[x * h + y] = tmp[(size_t)y * w + x];
    });
    return RT_OK;
}

int rt_select_rays_device(rt_scene* s, const rt_select_item* items, int32_t n_items, const rt_ray* d_rays, int64_t n,
                          rt_selection* d_out, void* stream)
{
    const char* name = "rt_select_rays_device";
    bool empty;
    int rc = check_rays(s, name, items, n_items, d_rays, n, d_out, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = prepare_items(s, name, items, n_items, (uint64_t)n, st);
    if (rc != RT_OK) return rc;
    rc = launch_rays(s, n_items, d_rays, n, d_out, st);
    if (rc != RT_OK) return rc;
    return end_op(s, st);
}

// A plain upload / launch / download per chunk, on the scene's own stream.
int rt_select_rays(rt_scene* s, const rt_select_item* items, int32_t n_items, const rt_ray* rays, int64_t n,
                   rt_selection* out)
{
    const char* name = "rt_select_rays";
    bool empty;
    int rc = check_rays(s, name, items, n_items, rays, n, out, &empty);
    if (rc != RT_OK || empty) return rc;
    hipStream_t st = s->stream;
    rc = prepare_items(s, name, items, n_items, (uint64_t)n, st);
    if (rc != RT_OK) return rc;
    const int64_t chunk = std::min(kSelectChunk, n);
    HIP_TRY(s->select_rays.reserve((size_t)chunk));
    HIP_TRY(s->select_out.reserve((size_t)chunk));
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        HIP_TRY(hipMemcpyAsync(s->select_rays.p, rays + a, (size_t)m * sizeof(rt_ray), hipMemcpyHostToDevice, st));
        rc = launch_rays(s, n_items, s->select_rays.p, m, s->select_out.p, st);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipMemcpyAsync(out + a, s->select_out.p, (size_t)m * sizeof(rt_selection), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return end_op(s, st);
}

int rt_debug_select_rays(const rt_prim* prims, int32_t n_prims, const rt_select_item* items, int32_t n_items,
                         const rt_ray* rays, int64_t n, rt_selection* out)
{
    const char* name = "rt_debug_select_rays";
    if (n_prims < 0) return bad_arg(name, "n_prims < 0");
    if (n_items < 0) return bad_arg(name, "n_items < 0");
    if (n < 0) return bad_arg(name, "n < 0");
    if ((n_prims > 0 && !prims) || (n_items > 0 && !items) || (n > 0 && (!rays || !out))) return bad_arg(name, "null pointer");
    for (int i = 0; i < n_prims; i++)
        if (prims[i].kind < 0 || prims[i].kind > 2) return bad_arg(name, "unknown primitive kind at index " + std::to_string(i));
    bool nodes;
    int rc = check_items(name, items, n_items, n_prims, (uint64_t)n, &nodes);
    if (rc != RT_OK) return rc;
    const std::vector<HostPrim> host = prepare_prims(prims, n_prims);
    RefBvh ref;
    if (nodes) {
        ref = build_ref_bvh(host);
        rc = check_nodes(name, items, n_items, (int)ref.nodes.size());
        if (rc != RT_OK) return rc;
    }
    std::vector<PrimD> pd;
    std::vector<XformD> xd;
    make_exact_records(host, pd, xd);
    DevScene sc{}; // the records select_items reads, in host memory
    sc.prims_d = pd.data();
    sc.xf_d = xd.data();
    sc.ref_nodes = ref.nodes.data();
    sc.n_ref_nodes = (int)ref.nodes.size();
    parallel_ranges((size_t)n, 256, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const rt_vec4d &ro = rays[i].origin, &rd = rays[i].direction;
            const Vec4d o{ro.x, ro.y, ro.z, ro.w}, d{rd.x, rd.y, rd.z, rd.w};
            out[i] = ray_valid_d(o, d) ? select_items(sc, items, n_items, o, d) : rt_selection{-1, 0, 0.0};
        }
    });
    return RT_OK;
}

} // extern "C"
