// probe_depth_host_check.cpp -- rt_debug_oct_texel_dirs, rt_debug_oct_texel, rt_debug_probe_depth_fold,
// rt_debug_probe_depth_close and rt_debug_shade_probes_depth under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc probe_depth_host_check_asan`;
// tests/test_probe_depth_host.py runs it).  Every array is allocated at its exact size so that a read or write
// past it is reported; what must hold whatever the numbers are is checked here, the numbers themselves against
// the replay in the Python test.  No device is touched.
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

static rt_probe_depth_params make_params(int sharpness, uint32_t flags)
{
    rt_probe_depth_params p;
    std::memset(&p, 0, sizeof p);
    p.d_max = 1.5;
    p.var_floor = 1e-3;
    p.sharpness = sharpness;
    p.flags = flags;
    return p;
}

static int check_texels()
{
    std::vector<double> T(64 * 3);
    if (rt_debug_oct_texel_dirs(T.data()) != RT_OK) return fail("rt_debug_oct_texel_dirs");
    std::vector<int32_t> t(64);
    if (rt_debug_oct_texel(T.data(), 64, t.data()) != RT_OK) return fail("rt_debug_oct_texel");
    for (int i = 0; i < 64; i++) {
        const double len2 = T[3 * i] * T[3 * i] + T[3 * i + 1] * T[3 * i + 1] + T[3 * i + 2] * T[3 * i + 2];
        if (t[i] != i || std::fabs(len2 - 1.0) > 1e-15) return fail("texel of its own direction", i, t[i]);
    }
    uint32_t s = 9;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> v(300 * 3);
    for (double& x : v) x = (unit(s) - 0.5) * std::ldexp(1.0, (int)(lcg(s) % 80u) - 40);
    v[0] = v[1] = v[2] = 0.0;
    v[3] = nan;
    v[8] = -inf;
    v[9] = -0.0, v[10] = -0.0, v[11] = -1e300;
    v[12] = 1e308, v[13] = -1e308, v[14] = 1e308; // (the 1-norm overflows)
    v[15] = 5e-324, v[16] = 0.0, v[17] = 0.0;
    std::vector<int32_t> out(300, 99);
    if (rt_debug_oct_texel(v.data(), 300, out.data()) != RT_OK) return fail("rt_debug_oct_texel, random");
    for (int i = 0; i < 300; i++)
        if (i < 3 ? out[i] != -1 : out[i] < 0 || out[i] > 63) return fail("texel range", i, out[i]);
    if (rt_debug_oct_texel(nullptr, 0, nullptr) != RT_OK || rt_debug_oct_texel(nullptr, 1, out.data()) != RT_ERR_ARG ||
        rt_debug_oct_texel(v.data(), 1, nullptr) != RT_ERR_ARG || rt_debug_oct_texel(v.data(), -1, out.data()) != RT_ERR_ARG ||
        rt_debug_oct_texel_dirs(nullptr) != RT_ERR_ARG)
        return fail("texel arguments");
    std::printf("ok texels\n");
    return 0;
}

static int check_fold_and_close()
{
    for (int sharpness : {0, 5, 8})
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)7})
            for (int32_t spp : {1, 5, 65}) {
                uint32_t s = 17u + (uint32_t)n * 3u + (uint32_t)spp + (uint32_t)sharpness;
                const rt_probe_depth_params P = make_params(sharpness, 0);
                const size_t m = (size_t)n * (size_t)spp;
                std::vector<rt_ray> rays(m);
                std::vector<rt_hit> hits(m);
                uint64_t want[4] = {0, 0, 0, 0};
                for (size_t j = 0; j < m; j++) {
                    std::memset(&rays[j], 0, sizeof(rt_ray));
                    std::memset(&hits[j], 0, sizeof(rt_hit));
                    double d[3] = {unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5};
                    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    const bool zero = j % 11 == 3 || !(len > 0);
                    rays[j].direction = zero ? rt_vec4d{0, 0, 0, 0} : rt_vec4d{(double)(float)(d[0] / len), (double)(float)(d[1] / len), (double)(float)(d[2] / len), 0};
                    hits[j].prim_id = j % 4 == 1 ? -1 : (int32_t)(j % 9);
                    hits[j].inside = j % 3 == 0;
                    hits[j].distance = hits[j].prim_id < 0 ? 0.0 : unit(s) * 3.0; // (half of them past d_max)
                    if (zero) want[3]++;
                    else if (hits[j].prim_id < 0) want[2]++;
                    else want[0]++, want[1] += hits[j].inside ? 1 : 0;
                }
                std::vector<rt_probe_depth> depth((size_t)n);
                std::vector<uint32_t> counts((size_t)n * 4, 0u);
                if (n) std::memset(depth.data(), 0, depth.size() * sizeof(rt_probe_depth));
                if (rt_debug_probe_depth_fold(&P, n ? rays.data() : nullptr, n ? hits.data() : nullptr, n, spp, n ? depth.data() : nullptr,
                                              n ? counts.data() : nullptr) != RT_OK)
                    return fail("rt_debug_probe_depth_fold", (long)n, spp);
                uint64_t got[4] = {0, 0, 0, 0};
                for (size_t i = 0; i < (size_t)n; i++) {
                    for (int k = 0; k < 4; k++) got[k] += counts[4 * i + k];
                    if (counts[4 * i] + counts[4 * i + 2] + counts[4 * i + 3] != (uint32_t)spp) return fail("counts of a probe", (long)n, (long)i);
                    for (int t = 0; t < 64; t++) {
                        const double s0 = depth[i].s[0][t], s1 = depth[i].s[1][t], s2 = depth[i].s[2][t];
                        if (!(s0 >= 0 && s1 >= 0 && s2 >= 0 && s1 <= s0 * P.d_max * (1 + 1e-12) && s2 <= s1 * P.d_max * (1 + 1e-12)))
                            return fail("sums of a texel", (long)i, t);
                    }
                }
                for (int k = 0; k < 4; k++)
                    if (got[k] != want[k]) return fail("counts", (long)n, k);
                std::vector<double> D((size_t)n * 128, -7.0);
                if (rt_debug_probe_depth_close(n ? depth.data() : nullptr, n, n ? D.data() : nullptr) != RT_OK)
                    return fail("rt_debug_probe_depth_close", (long)n, spp);
                for (size_t i = 0; i < (size_t)n; i++)
                    for (int t = 0; t < 64; t++) {
                        const double mu = D[(i * 64 + t) * 2], m2 = D[(i * 64 + t) * 2 + 1];
                        if (depth[i].s[0][t] > 0 ? !(mu >= 0 && mu <= P.d_max * (1 + 1e-12) && m2 >= 0) : !(std::isnan(mu) && std::isnan(m2)))
                            return fail("closed texel", (long)i, t);
                    }
            }
    // argument errors, the outputs untouched
    rt_probe_depth_params P = make_params(5, 0);
    rt_ray r;
    rt_hit h;
    std::memset(&r, 0, sizeof r);
    std::memset(&h, 0, sizeof h);
    r.direction.z = 1;
    rt_probe_depth d;
    for (auto& row : d.s)
        for (double& x : row) x = -7.0;
    uint32_t c[4] = {7, 7, 7, 7};
    double D[128];
    for (double& x : D) x = -7.0;
    rt_probe_depth_params bad[9];
    for (rt_probe_depth_params& b : bad) b = P;
    bad[0].d_max = 0, bad[1].d_max = std::numeric_limits<double>::infinity(), bad[2].d_max = std::numeric_limits<double>::quiet_NaN();
    bad[3].var_floor = 0, bad[4].var_floor = -1, bad[5].sharpness = -1, bad[6].sharpness = 9, bad[7].flags = 2, bad[8].reserved[1] = 1;
    for (const rt_probe_depth_params& b : bad)
        if (rt_debug_probe_depth_fold(&b, &r, &h, 1, 1, &d, c) != RT_ERR_ARG) return fail("params rules", (long)(&b - bad));
    if (rt_debug_probe_depth_fold(nullptr, &r, &h, 1, 1, &d, c) != RT_ERR_ARG || rt_debug_probe_depth_fold(&P, nullptr, &h, 1, 1, &d, c) != RT_ERR_ARG ||
        rt_debug_probe_depth_fold(&P, &r, nullptr, 1, 1, &d, c) != RT_ERR_ARG || rt_debug_probe_depth_fold(&P, &r, &h, 1, 1, nullptr, c) != RT_ERR_ARG ||
        rt_debug_probe_depth_fold(&P, &r, &h, 1, 1, &d, nullptr) != RT_ERR_ARG || rt_debug_probe_depth_fold(&P, &r, &h, -1, 1, &d, c) != RT_ERR_ARG ||
        rt_debug_probe_depth_fold(&P, &r, &h, 1, 0, &d, c) != RT_ERR_ARG || rt_debug_probe_depth_fold(&P, nullptr, nullptr, 0, 1, nullptr, nullptr) != RT_OK ||
        rt_debug_probe_depth_close(nullptr, 1, D) != RT_ERR_ARG || rt_debug_probe_depth_close(&d, 1, nullptr) != RT_ERR_ARG ||
        rt_debug_probe_depth_close(&d, -1, D) != RT_ERR_ARG || rt_debug_probe_depth_close(nullptr, 0, nullptr) != RT_OK)
        return fail("fold and close arguments");
    if (d.s[0][0] != -7 || d.s[2][63] != -7 || c[0] != 7 || c[3] != 7 || D[0] != -7 || D[127] != -7) return fail("outputs touched");
    std::printf("ok fold and close\n");
    return 0;
}

static rt_probe_grid make_grid(int nx, int ny, int nz)
{
    rt_probe_grid g;
    std::memset(&g, 0, sizeof g);
    const double origin[3] = {-1.0, 0.5, 2.0}, step[3] = {0.5, 0.75, 1.25};
    for (int a = 0; a < 3; a++) g.origin[a] = origin[a], g.step[a] = step[a];
    g.dims[0] = nx, g.dims[1] = ny, g.dims[2] = nz;
    g.bias = 0.25;
    return g;
}

static int check_shade()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {1, 3, 1}};
    for (const int* dm : shapes)
        for (uint32_t flags : {0u, RT_PROBE_DEPTH_WRAP})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)200}) {
                uint32_t s = 41u + (uint32_t)n + (uint32_t)dm[1] * 7u + flags;
                const rt_probe_grid g = make_grid(dm[0], dm[1], dm[2]);
                const rt_probe_depth_params P = make_params(5, flags);
                const size_t np = (size_t)dm[0] * dm[1] * dm[2];
                std::vector<rt_surfel> pts((size_t)n);
                for (size_t i = 0; i < pts.size(); i++) {
                    double p[3], nrm[3];
                    for (int a = 0; a < 3; a++) {
                        const double span = g.dims[a] > 1 ? (g.dims[a] - 1) * g.step[a] : g.step[a];
                        p[a] = g.origin[a] - 0.4 * span + unit(s) * 1.8 * span;
                        if (i % 4 == 1) p[a] = g.origin[a] + (double)(lcg(s) % (uint32_t)g.dims[a]) * g.step[a]; // on a probe
                        nrm[a] = (unit(s) - 0.5) * 6;
                    }
                    if (i % 16 == 5) nrm[0] = nrm[1] = 0, nrm[2] = 1, p[2] -= g.bias; // the bias puts it on the probe
                    pts[i].position = {p[0], p[1], p[2], 1};
                    pts[i].normal = {nrm[0], nrm[1], nrm[2], 0};
                    if (i % 50 == 7) pts[i].position.y = nan;
                    if (i % 50 == 30) pts[i].normal.x = inf;
                    if (i % 50 == 14) pts[i].normal = {0, 0, 0, 0};
                }
                std::vector<double> L(np * 27), D(np * 128);
                for (double& v : L) v = unit(s) * 2 - 0.5;
                if (np > 1) L[27 * (np - 1) + 13] = nan; // an absent probe
                for (size_t j = 0; j < np * 64; j++) {
                    const double mu = 0.1 + unit(s) * 1.6;
                    D[2 * j] = j % 7 == 2 ? nan : mu;
                    D[2 * j + 1] = j % 7 == 2 ? nan : mu * mu + unit(s) * 0.2 - 0.01;
                }
                std::vector<rt_color> E((size_t)n, rt_color{-7, -7, -7});
                std::vector<double> w((size_t)n, -7.0);
                for (int pass = 0; pass < 2; pass++) { // with and without a weight array
                    if (rt_debug_shade_probes_depth(&g, &P, n ? L.data() : nullptr, n ? D.data() : nullptr, n ? pts.data() : nullptr, n,
                                                    n ? E.data() : nullptr, pass || !n ? nullptr : w.data()) != RT_OK)
                        return fail("rt_debug_shade_probes_depth", (long)n, pass);
                    for (size_t i = 0; i < (size_t)n; i++) {
                        if (!(w[i] >= 0.0 && w[i] <= 1.2 * (1.0 + 1e-15))) return fail("weight range", (long)n, (long)i);
                        if (!std::isfinite(E[i].r) || !std::isfinite(E[i].g) || !std::isfinite(E[i].b)) return fail("irradiance finite", (long)n, (long)i);
                        if (w[i] == 0.0 && (E[i].r != 0 || E[i].g != 0 || E[i].b != 0)) return fail("zeros of a point without a probe", (long)n, (long)i);
                    }
                }
            }
    // argument errors, the outputs untouched
    rt_probe_grid g = make_grid(4, 3, 2);
    rt_probe_depth_params P = make_params(5, 0);
    rt_surfel p;
    std::memset(&p, 0, sizeof p);
    p.normal.z = 1;
    std::vector<double> L(24 * 27, 1.0), D(24 * 128, 1.0);
    double w = -7;
    rt_color E = {-7, -7, -7};
    rt_probe_grid bad[6];
    for (rt_probe_grid& b : bad) b = g;
    bad[0].step[1] = 0, bad[1].origin[2] = inf, bad[2].dims[0] = 0, bad[3].flags = RT_PROBE_GRID_VISIBILITY, bad[4].flags = 2, bad[5].reserved[0] = 1;
    for (const rt_probe_grid& b : bad)
        if (rt_debug_shade_probes_depth(&b, &P, L.data(), D.data(), &p, 1, &E, &w) != RT_ERR_ARG) return fail("grid rules", (long)(&b - bad));
    rt_probe_depth_params badp = P;
    badp.var_floor = 0;
    if (rt_debug_shade_probes_depth(&g, &badp, L.data(), D.data(), &p, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, nullptr, L.data(), D.data(), &p, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(nullptr, &P, L.data(), D.data(), &p, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, nullptr, D.data(), &p, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, L.data(), nullptr, &p, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, L.data(), D.data(), nullptr, 1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, L.data(), D.data(), &p, 1, nullptr, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, L.data(), D.data(), &p, -1, &E, &w) != RT_ERR_ARG ||
        rt_debug_shade_probes_depth(&g, &P, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != RT_OK)
        return fail("shade arguments");
    if (E.r != -7 || E.g != -7 || E.b != -7 || w != -7) return fail("outputs touched");
    std::printf("ok shade\n");
    return 0;
}

int main()
{
    if (check_texels()) return 1;
    if (check_fold_and_close()) return 1;
    if (check_shade()) return 1;
    std::printf("probe_depth_host_check: ok\n");
    return 0;
}
