// reproject_host_check.cpp -- the temporal reprojection's host twin under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc reproject_host_check_asan`;
// tests/test_reproject_host.py runs it): rt_debug_reproject over the identity move on the frames 8 x 8,
// 37 x 19 and 130 x 70 (a plane seen by a frustum camera, rays from rt_camera_rays), each also with a
// plane stride beyond the frame and with and without out_src and the cap; each rejection of the header on
// a hand-made 8 x 8 pair of hit arrays; the argument errors.  Every array is allocated at its exact size
// so that a read or write past it is reported.  No device is touched.  Prints one "ok ..." line per part.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rtcore.h"

static int fail(const char* what, long a = 0, long b = 0)
{
    std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (double)(lcg(s) >> 8) * (1.0 / 16777216.0); }

struct Acc {
    std::vector<double> sum, q;
    std::vector<uint32_t> ns, nm, nb;
    size_t n, plane;
    Acc(size_t n_, size_t pad, uint32_t seed, uint32_t n_max) : n(n_), plane(n_ + pad)
    {
        sum.assign(2 * plane + n, -7.0);
        q.resize(n), ns.resize(n), nm.resize(n), nb.resize(n);
        for (size_t i = 0; i < n; i++) {
            const uint32_t N = lcg(seed) % 9 == 0 ? 0 : 1 + lcg(seed) % n_max;
            ns[i] = N ? lcg(seed) % (N + 1) : 0;
            nm[i] = N - ns[i];
            nb[i] = lcg(seed) % (N + 1);
            for (int c = 0; c < 3; c++) sum[c * plane + i] = unit(seed) * 3.0 * ns[i];
            q[i] = unit(seed) * 50.0;
        }
    }
};
struct Out {
    std::vector<double> sum, q;
    std::vector<uint32_t> ns, nm, nb;
    std::vector<int32_t> src;
    explicit Out(const Acc& a) : sum(a.sum.size(), -7.0), q(a.n, -7.0), ns(a.n, 7u), nm(a.n, 7u), nb(a.n, 7u), src(a.n, 7) {}
};

static int run(const rt_reproject_params& P, const rt_camera& cam, const std::vector<rt_hit>& prev, const std::vector<rt_hit>& cur,
               const Acc& a, int w, int h, Out& o, bool with_src = true)
{
    return rt_debug_reproject(&P, &cam, prev.data(), cur.data(), a.sum.data(), a.ns.data(), a.nm.data(), a.q.data(), a.nb.data(),
                              a.plane == a.n ? 0 : a.plane, w, h, o.sum.data(), o.ns.data(), o.nm.data(), o.q.data(), o.nb.data(),
                              with_src ? o.src.data() : nullptr);
}

static bool same_pixel(const Acc& a, size_t s, const Out& o, size_t p)
{
    for (int c = 0; c < 3; c++)
        if (std::memcmp(&a.sum[c * a.plane + s], &o.sum[c * a.plane + p], 8) != 0) return false;
    return std::memcmp(&a.q[s], &o.q[p], 8) == 0 && a.ns[s] == o.ns[p] && a.nm[s] == o.nm[p] && a.nb[s] == o.nb[p];
}
static bool empty_pixel(const Acc& a, const Out& o, size_t p)
{
    const double z = 0.0;
    for (int c = 0; c < 3; c++)
        if (std::memcmp(&z, &o.sum[c * a.plane + p], 8) != 0) return false;
    return std::memcmp(&z, &o.q[p], 8) == 0 && o.ns[p] == 0 && o.nm[p] == 0 && o.nb[p] == 0;
}

static int frames()
{
    const int sizes[][2] = {{8, 8}, {37, 19}, {130, 70}};
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.kind = RT_CAMERA_FRUSTUM;
    cam.position = {0.25, -0.5, 0, 1};
    cam.look_at = {0.5, 0.25, 4, 1};
    cam.up = {0, 1, 0, 0};
    cam.fov_y = 1.2;
    for (const auto& f : sizes) {
        const int w = f[0], h = f[1];
        const size_t n = (size_t)w * h;
        std::vector<rt_ray> rays(n); // [x * h + y]
        if (rt_camera_rays(&cam, w, h, 0, 0, w, h, rays.data()) != RT_OK) return fail("rt_camera_rays", w, h);
        std::vector<rt_hit> hits(n);
        std::memset(hits.data(), 0, n * sizeof(rt_hit));
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                rt_hit& H = hits[(size_t)y * w + x];
                const rt_ray& r = rays[(size_t)x * h + y];
                H.prim_id = y == 0 ? -1 : 1; // the top row: no hit
                if (H.prim_id < 0) continue;
                const double t = (5.0 - r.origin.z) / r.direction.z; // the plane z = 5
                H.distance = t;
                H.position[0] = (float)(r.origin.x + t * r.direction.x);
                H.position[1] = (float)(r.origin.y + t * r.direction.y);
                H.position[2] = 5.0f;
                H.normal[2] = -1.0f;
            }
        for (size_t pad : {(size_t)0, (size_t)37})
            for (uint32_t max_history : {1000u, 12u})
                for (bool with_src : {true, false}) {
                    const Acc a(n, pad, 977u + (uint32_t)n, 40);
                    Out o(a);
                    const rt_reproject_params P{0.05f, 0.9f, max_history, RT_REPROJECT_SAME_PRIM, {0, 0, 0, 0}};
                    if (run(P, cam, hits, hits, a, w, h, o, with_src) != RT_OK) return fail("call", w, h);
                    for (size_t p = 0; p < n; p++) {
                        const uint64_t N = (uint64_t)a.ns[p] + a.nm[p];
                        const bool accepted = hits[p].prim_id >= 0 && N > 0;
                        if (with_src && o.src[p] != (accepted ? (int32_t)p : -1)) return fail("src", (long)p, o.src[p]);
                        if (!with_src && o.src[p] != 7) return fail("out_src written", (long)p);
                        if (!accepted) {
                            if (!empty_pixel(a, o, p)) return fail("empty pixel", (long)p);
                        } else if (N <= max_history) {
                            if (!same_pixel(a, p, o, p)) return fail("copy", (long)p);
                        } else if ((uint64_t)o.ns[p] + o.nm[p] != max_history || o.nb[p] > a.nb[p]) {
                            return fail("cap", (long)p);
                        }
                    }
                    for (size_t i = n; i < a.plane; i++)
                        if (o.sum[i] != -7.0 || o.sum[a.plane + i] != -7.0) return fail("padding written", (long)i);
                }
    }
    std::printf("ok reproject %zu frames\n", sizeof(sizes) / sizeof(sizes[0]));
    return 0;
}

// An axis-aligned ortho camera with h_mult = 1 and v_mult = -1 over 8 x 8: fx = 4 + a, fy = 4 - b exactly.
static int rejections()
{
    const int w = 8, h = 8;
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.kind = RT_CAMERA_ORTHO;
    cam.position = {0, 0, 0, 1};
    cam.look_at = {0, 0, 1, 1};
    cam.up = {0, 1, 0, 0};
    cam.size_mult = 4.0;
    std::vector<rt_ray> rays(64);
    if (rt_camera_rays(&cam, w, h, 0, 0, w, h, rays.data()) != RT_OK) return fail("rt_camera_rays");
    std::vector<rt_hit> base(64);
    std::memset(base.data(), 0, 64 * sizeof(rt_hit));
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            rt_hit& H = base[(size_t)y * w + x];
            const rt_ray& r = rays[(size_t)x * h + y];
            H.distance = 5.0;
            H.position[0] = (float)r.origin.x, H.position[1] = (float)r.origin.y, H.position[2] = 5.0f;
            H.normal[2] = -1.0f;
        }
    std::vector<rt_hit> cur = base, prev = base;
    Acc a(64, 0, 5u, 40);
    for (size_t i = 0; i < 64; i++)
        if (a.ns[i] + a.nm[i] == 0) a.ns[i] = 1;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the step between the columns' positions, whatever the sign of `side`
    const float dx = base[1].position[0] - base[0].position[0];
    bool reject[64] = {};
    auto no = [&](int x, int y) { reject[y * w + x] = true; };
    cur[0].prim_id = -1, no(0, 0);
    cur[1].position[1] = inf, no(1, 0);
    cur[2].position[0] = nan, no(2, 0);
    cur[3].position[2] = 0.0f, no(3, 0);
    cur[4].position[2] = -5.0f, no(4, 0);
    cur[8 + 1].position[0] = base[0].position[0] - 0.5f * dx - 0.001f * dx, no(1, 1); // left of the frame
    cur[8 + 2].position[0] = base[7].position[0] + 0.5f * dx, no(2, 1);               // fx = 7.5
    prev[16 + 0].prim_id = -1, no(0, 2);
    prev[16 + 1].prim_id = 3, no(1, 2);
    prev[16 + 2].inside = 1, no(2, 2);
    cur[16 + 3].normal[0] = 0.6f, cur[16 + 3].normal[2] = -0.8f, no(3, 2);
    cur[16 + 5].normal[1] = nan, no(5, 2);
    prev[24 + 1].position[2] = 5.26f, no(1, 3);
    a.ns[32] = a.nm[32] = 0, no(0, 4);
    Out o(a);
    const rt_reproject_params P{0.05f, 0.9f, 1000u, RT_REPROJECT_SAME_PRIM, {0, 0, 0, 0}};
    if (run(P, cam, prev, cur, a, w, h, o) != RT_OK) return fail("call");
    for (int p = 0; p < 64; p++) {
        if (o.src[p] != (reject[p] ? -1 : p)) return fail("decision", p, o.src[p]);
        if (reject[p] ? !empty_pixel(a, o, (size_t)p) : !same_pixel(a, (size_t)p, o, (size_t)p)) return fail("outputs", p);
    }
    std::printf("ok rejections\n");
    return 0;
}

static int arguments()
{
    const Acc a(64, 0, 1u, 40);
    Out o(a);
    std::vector<rt_hit> hits(64);
    std::memset(hits.data(), 0, 64 * sizeof(rt_hit));
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.position = {0, 0, 0, 1}, cam.look_at = {0, 0, 1, 1}, cam.up = {0, 1, 0, 0}, cam.fov_y = 1.0;
    rt_reproject_params P{0.05f, 0.9f, 32u, RT_REPROJECT_SAME_PRIM, {0, 0, 0, 0}};
    if (run(P, cam, hits, hits, a, 8, 8, o) != RT_OK) return fail("good call");
    if (rt_debug_reproject(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 8, 8, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr) != RT_ERR_ARG)
        return fail("null arguments");
    if (rt_debug_reproject(&P, &cam, hits.data(), hits.data(), a.sum.data(), a.ns.data(), a.nm.data(), a.q.data(), a.nb.data(), 0, 8, 8,
                           const_cast<double*>(a.sum.data()), o.ns.data(), o.nm.data(), o.q.data(), o.nb.data(), nullptr) != RT_ERR_ARG)
        return fail("in place");
    P.max_history = 0;
    if (run(P, cam, hits, hits, a, 8, 8, o) != RT_ERR_ARG) return fail("max_history");
    P.max_history = 32, P.sigma_z = std::numeric_limits<float>::quiet_NaN();
    if (run(P, cam, hits, hits, a, 8, 8, o) != RT_ERR_ARG) return fail("sigma_z");
    P.sigma_z = 0.05f, P.reserved[3] = 1;
    if (run(P, cam, hits, hits, a, 8, 8, o) != RT_ERR_ARG) return fail("reserved");
    P.reserved[3] = 0, cam.kind = 2;
    if (run(P, cam, hits, hits, a, 8, 8, o) != RT_ERR_ARG) return fail("camera kind");
    std::printf("ok arguments\n");
    return 0;
}

int main()
{
    if (frames()) return 1;
    if (rejections()) return 1;
    if (arguments()) return 1;
    return 0;
}
