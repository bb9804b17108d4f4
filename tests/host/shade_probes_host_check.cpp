// shade_probes_host_check.cpp -- rt_debug_probe_radiance, rt_debug_probe_segments and rt_debug_shade_probes
// under AddressSanitizer and UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc
// shade_probes_host_check_asan`; tests/test_shade_probes_host.py runs it).  Every array is allocated at its
// exact size so that a read or write past it is reported: the grids 4 x 3 x 2, 1 x 1 x 1 and 1 x 3 x 1 over
// n = 0, 1, 63 and 200 points, inside and outside the grid, on probes and on cell faces, with invalid points,
// absent probes, random answers and none; what must hold whatever the numbers are is checked here, the
// numbers themselves against the replay in the Python test.  No device is touched.
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

static rt_probe_grid make_grid(int nx, int ny, int nz, uint32_t flags)
{
    rt_probe_grid g;
    std::memset(&g, 0, sizeof g);
    const double origin[3] = {-1.0, 0.5, 2.0}, step[3] = {0.5, 0.75, 1.25};
    for (int a = 0; a < 3; a++) g.origin[a] = origin[a], g.step[a] = step[a];
    g.dims[0] = nx, g.dims[1] = ny, g.dims[2] = nz;
    g.flags = flags;
    g.bias = 0.25;
    return g;
}

static bool all_zero(const void* p, size_t bytes)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; i++)
        if (b[i]) return false;
    return true;
}

static int check_radiance()
{
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)65}) {
        uint32_t s = 3u + (uint32_t)n;
        std::vector<rt_probe_sh> sh((size_t)n);
        std::vector<uint32_t> ns((size_t)n), nm((size_t)n);
        std::vector<double> L((size_t)n * 27, -7.0);
        for (size_t i = 0; i < (size_t)n; i++) {
            for (int l = 0; l < 9; l++)
                for (int j = 0; j < 4; j++) sh[i].c[l][j] = unit(s) * 8 - 4;
            ns[i] = i % 5 ? lcg(s) : 0u; // (sums past 32 bits among them)
            nm[i] = i % 5 ? lcg(s) : 0u;
        }
        const rt_color ambient = {0.2, 0.3, 0.4};
        if (rt_debug_probe_radiance(n ? sh.data() : nullptr, n ? ns.data() : nullptr, n ? nm.data() : nullptr, n, ambient,
                                    n ? L.data() : nullptr) != RT_OK)
            return fail("rt_debug_probe_radiance", (long)n);
        for (size_t i = 0; i < (size_t)n; i++) {
            const double N = (double)((uint64_t)ns[i] + (uint64_t)nm[i]);
            for (int l = 0; l < 9; l++)
                for (int ch = 0; ch < 3; ch++) {
                    const double got = L[i * 27 + 3 * l + ch], amb = ch == 0 ? ambient.r : ch == 1 ? ambient.g : ambient.b;
                    if (N == 0 ? !std::isnan(got) : got != ((4.0 * 3.141592653589793) / N) * (sh[i].c[l][ch] + sh[i].c[l][3] * amb))
                        return fail("radiance bits", (long)i, l);
                }
        }
    }
    rt_probe_sh sh;
    std::memset(&sh, 0, sizeof sh);
    uint32_t a = 1;
    double L[27];
    const rt_color amb = {0, 0, 0};
    if (rt_debug_probe_radiance(&sh, &a, &a, -1, amb, L) != RT_ERR_ARG || rt_debug_probe_radiance(nullptr, &a, &a, 1, amb, L) != RT_ERR_ARG ||
        rt_debug_probe_radiance(&sh, nullptr, &a, 1, amb, L) != RT_ERR_ARG || rt_debug_probe_radiance(&sh, &a, nullptr, 1, amb, L) != RT_ERR_ARG ||
        rt_debug_probe_radiance(&sh, &a, &a, 1, amb, nullptr) != RT_ERR_ARG)
        return fail("radiance arguments");
    std::printf("ok radiance\n");
    return 0;
}

static void make_points(const rt_probe_grid& g, std::vector<rt_surfel>& pts, uint32_t& s)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < pts.size(); i++) {
        double p[3], nrm[3];
        for (int a = 0; a < 3; a++) {
            const double span = g.dims[a] > 1 ? (g.dims[a] - 1) * g.step[a] : g.step[a];
            p[a] = g.origin[a] - 0.4 * span + unit(s) * 1.8 * span;
            if (i % 4 == 1) p[a] = g.origin[a] + (double)(lcg(s) % (uint32_t)g.dims[a]) * g.step[a]; // on a probe
            if (i % 4 == 2 && a == (int)(i % 3)) p[a] = g.origin[a] + (double)(lcg(s) % (uint32_t)g.dims[a]) * g.step[a];
            nrm[a] = (unit(s) - 0.5) * 6;
        }
        if (i % 16 == 5) nrm[0] = nrm[1] = 0, nrm[2] = 1, p[2] -= g.bias; // the bias puts it on the probe
        pts[i].position = {p[0], p[1], p[2], 1};
        pts[i].normal = {nrm[0], nrm[1], nrm[2], 0};
        if (i % 50 == 7) pts[i].position.y = nan;
        if (i % 50 == 30) pts[i].normal.x = inf;
        if (i % 50 == 14) pts[i].normal = {0, 0, 0, 0};
        if (i % 50 == 21) pts[i].position.w = -inf;
    }
}

static bool valid(const rt_surfel& p)
{
    const double v[8] = {p.position.x, p.position.y, p.position.z, p.position.w, p.normal.x, p.normal.y, p.normal.z, p.normal.w};
    for (double x : v)
        if (!std::isfinite(x)) return false;
    const double n2 = (v[4] * v[4] + v[5] * v[5]) + v[6] * v[6];
    return n2 != 0 && std::isfinite(n2);
}

static int check_grids()
{
    const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {1, 3, 1}};
    for (const int* d : shapes)
        for (uint32_t flags : {RT_PROBE_GRID_VISIBILITY, 0u})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)200}) {
                uint32_t s = 41u + (uint32_t)n + (uint32_t)d[1] * 7u + flags;
                const rt_probe_grid g = make_grid(d[0], d[1], d[2], flags);
                const size_t np = (size_t)d[0] * d[1] * d[2];
                std::vector<rt_surfel> pts((size_t)n);
                make_points(g, pts, s);
                std::vector<double> L(np * 27);
                for (double& v : L) v = unit(s) * 2 - 0.5;
                if (np > 1) L[27 * (np - 1) + 13] = std::numeric_limits<double>::quiet_NaN(); // an absent probe
                std::vector<rt_ray> rays((size_t)n * 8);
                std::vector<double> t_max((size_t)n * 8, -7.0), w((size_t)n, -7.0);
                std::vector<uint8_t> occ((size_t)n * 8);
                for (uint8_t& o : occ) o = (uint8_t)(lcg(s) >> 31);
                std::vector<rt_color> E((size_t)n, rt_color{-7, -7, -7});
                if (n) std::memset(rays.data(), 0x5a, rays.size() * sizeof(rt_ray));
                if (rt_debug_probe_segments(&g, n ? pts.data() : nullptr, n, n ? rays.data() : nullptr, n ? t_max.data() : nullptr) != RT_OK)
                    return fail("rt_debug_probe_segments", (long)n, d[1]);
                for (size_t j = 0; j < (size_t)n * 8; j++) {
                    const bool empty = all_zero(&rays[j], sizeof(rt_ray));
                    if (empty != (t_max[j] == 0.0) || (!empty && !(t_max[j] > 0.0 && rays[j].origin.w == 1.0 && rays[j].direction.w == 0.0)))
                        return fail("segment form", (long)n, (long)j);
                    if (!empty && (!flags || !valid(pts[j / 8]))) return fail("segment of an invalid point or without the flag", (long)n, (long)j);
                }
                for (int pass = 0; pass < 3; pass++) { // answers, none, and no weight wanted
                    if (rt_debug_shade_probes(&g, n ? L.data() : nullptr, n ? pts.data() : nullptr, n, pass == 0 && n ? occ.data() : nullptr,
                                              n ? E.data() : nullptr, pass == 2 || !n ? nullptr : w.data()) != RT_OK)
                        return fail("rt_debug_shade_probes", (long)n, pass);
                    for (size_t i = 0; i < (size_t)n; i++) {
                        if (!(w[i] >= 0.0 && w[i] <= 1.0 + 1e-15)) return fail("weight range", (long)n, (long)i);
                        if (!std::isfinite(E[i].r) || !std::isfinite(E[i].g) || !std::isfinite(E[i].b)) return fail("irradiance finite", (long)n, (long)i);
                        if ((!valid(pts[i]) || w[i] == 0.0) && (E[i].r != 0 || E[i].g != 0 || E[i].b != 0 || w[i] != 0))
                            return fail("zeros of a point without a probe", (long)n, (long)i);
                    }
                }
            }
    // argument errors, the outputs untouched
    rt_probe_grid g = make_grid(4, 3, 2, 1u);
    rt_surfel p;
    std::memset(&p, 0, sizeof p);
    p.normal.z = 1;
    std::vector<double> L(24 * 27, 1.0);
    rt_ray r[8];
    double t[8], w = -7;
    rt_color E = {-7, -7, -7};
    std::memset(r, 0x5a, sizeof r);
    rt_probe_grid bad[8];
    for (rt_probe_grid& b : bad) b = g;
    bad[0].step[1] = 0, bad[1].origin[2] = std::numeric_limits<double>::infinity(), bad[2].dims[0] = 0, bad[3].dims[0] = 1 << 30, bad[3].dims[1] = 2;
    bad[4].bias = -1, bad[5].flags = 2, bad[6].reserved[0] = 1, bad[7].step[0] = std::numeric_limits<double>::quiet_NaN();
    for (const rt_probe_grid& b : bad)
        if (rt_debug_probe_segments(&b, &p, 1, r, t) != RT_ERR_ARG || rt_debug_shade_probes(&b, L.data(), &p, 1, nullptr, &E, &w) != RT_ERR_ARG)
            return fail("grid rules", (long)(&b - bad));
    if (rt_debug_probe_segments(nullptr, &p, 1, r, t) != RT_ERR_ARG || rt_debug_probe_segments(&g, &p, -1, r, t) != RT_ERR_ARG ||
        rt_debug_probe_segments(&g, nullptr, 1, r, t) != RT_ERR_ARG || rt_debug_probe_segments(&g, &p, 1, nullptr, t) != RT_ERR_ARG ||
        rt_debug_probe_segments(&g, &p, 1, r, nullptr) != RT_ERR_ARG || rt_debug_shade_probes(nullptr, L.data(), &p, 1, nullptr, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes(&g, nullptr, &p, 1, nullptr, &E, &w) != RT_ERR_ARG || rt_debug_shade_probes(&g, L.data(), nullptr, 1, nullptr, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes(&g, L.data(), &p, 1, nullptr, nullptr, &w) != RT_ERR_ARG || rt_debug_shade_probes(&g, L.data(), &p, -1, nullptr, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes(&g, nullptr, nullptr, 0, nullptr, nullptr, nullptr) != RT_OK || rt_debug_probe_segments(&g, nullptr, 0, nullptr, nullptr) != RT_OK)
        return fail("arguments");
    if (E.r != -7 || E.g != -7 || E.b != -7 || w != -7 || reinterpret_cast<unsigned char*>(r)[0] != 0x5a) return fail("outputs touched");
    std::printf("ok grids\n");
    return 0;
}

int main()
{
    if (check_radiance()) return 1;
    if (check_grids()) return 1;
    std::printf("shade_probes_host_check: ok\n");
    return 0;
}
