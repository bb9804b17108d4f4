// probe_relocate_host_check.cpp -- rt_debug_probe_positions, rt_debug_probe_relocate,
// rt_debug_probe_segments_placed, rt_debug_shade_probes_placed and rt_debug_shade_probes_depth_placed under
// AddressSanitizer and UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc probe_relocate_host_check_asan`;
// tests/test_probe_relocate_host.py runs it).  Every array is allocated at its exact size so that a read or write
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
static const double inf = std::numeric_limits<double>::infinity(), nan_ = std::numeric_limits<double>::quiet_NaN();

static rt_probe_grid make_grid(int nx, int ny, int nz, uint32_t flags)
{
    rt_probe_grid g;
    std::memset(&g, 0, sizeof g);
    const double origin[3] = {-1.0, 0.5, 2.0}, step[3] = {0.5, 0.75, 1.25};
    for (int a = 0; a < 3; a++) g.origin[a] = origin[a], g.step[a] = step[a];
    g.dims[0] = nx, g.dims[1] = ny, g.dims[2] = nz;
    g.bias = 0.25;
    g.flags = flags;
    return g;
}

static rt_probe_relocate_params make_params(uint32_t flags)
{
    rt_probe_relocate_params p;
    std::memset(&p, 0, sizeof p);
    p.back_share = 0.25;
    p.min_front = 0.3;
    p.max_offset = 0.45;
    p.flags = flags;
    return p;
}

static int check_relocate()
{
    const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {5, 1, 1}};
    for (const int* dm : shapes)
        for (uint32_t flags : {0u, RT_PROBE_RELOCATE_CLASSIFY_ONLY})
            for (int32_t spp : {1, 5, 65}) {
                uint32_t s = 23u + (uint32_t)dm[0] * 5u + (uint32_t)spp + flags;
                const rt_probe_grid g = make_grid(dm[0], dm[1], dm[2], 0);
                const rt_probe_relocate_params P = make_params(flags);
                const size_t n = (size_t)dm[0] * dm[1] * dm[2], m = n * (size_t)spp;
                std::vector<rt_ray> rays(m);
                std::vector<rt_hit> hits(m);
                for (size_t j = 0; j < m; j++) {
                    std::memset(&rays[j], 0, sizeof(rt_ray));
                    std::memset(&hits[j], 0, sizeof(rt_hit));
                    double d[3] = {unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5};
                    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    const bool zero = j % 11 == 3 || !(len > 0);
                    rays[j].direction = zero ? rt_vec4d{0, 0, 0, 0} : rt_vec4d{(double)(float)(d[0] / len), (double)(float)(d[1] / len), (double)(float)(d[2] / len), 0};
                    hits[j].prim_id = j % 4 == 1 ? -1 : (int32_t)(j % 9);
                    hits[j].inside = j % 3 == 0;
                    hits[j].distance = hits[j].prim_id < 0 ? 0.0 : j % 17 == 6 ? nan_ : unit(s) * 1.5;
                }
                std::vector<double> offsets(n * 3);
                for (size_t i = 0; i < n; i++)
                    for (int a = 0; a < 3; a++) offsets[3 * i + a] = (unit(s) - 0.5) * 0.4 * g.step[a];
                if (n > 2) offsets[3 * 2 + 1] = nan_;
                const std::vector<double> before = offsets;
                std::vector<rt_probe_relocation> info(n);
                std::memset(info.data(), 0x55, n * sizeof(rt_probe_relocation));
                if (rt_debug_probe_relocate(&g, &P, rays.data(), hits.data(), spp, offsets.data(), info.data()) != RT_OK)
                    return fail("rt_debug_probe_relocate", (long)n, spp);
                for (size_t i = 0; i < n; i++) {
                    const rt_probe_relocation& r = info[i];
                    if (r.front + r.back + r.misses + r.skipped != (uint32_t)spp || r.reserved != 0 || (r.state & ~3u) || r.moved > 1u)
                        return fail("record of a probe", (long)n, (long)i);
                    if (r.k_near < -1 || r.k_near >= spp || r.k_back < -1 || r.k_back >= spp || r.k_far < -1 || r.k_far >= spp)
                        return fail("winner range", (long)n, (long)i);
                    if ((r.k_near < 0) != (r.d_near == inf) || (r.k_back < 0) != (r.d_back == inf) || (r.k_far < 0) != (r.d_far == -inf))
                        return fail("winner and distance", (long)n, (long)i);
                    const bool same = !std::memcmp(&offsets[3 * i], &before[3 * i], 3 * sizeof(double));
                    if (flags ? !same : same == (r.moved != 0u)) return fail("moved", (long)n, (long)i);
                    double e2 = 0;
                    for (int a = 0; a < 3; a++) e2 += (offsets[3 * i + a] / g.step[a]) * (offsets[3 * i + a] / g.step[a]);
                    if (!flags && r.moved && !(e2 < 0.45 * 0.45)) return fail("an accepted offset lies inside the ellipsoid", (long)n, (long)i);
                }
                std::vector<rt_surfel> probes(n);
                if (rt_debug_probe_positions(&g, offsets.data(), probes.data()) != RT_OK) return fail("rt_debug_probe_positions", (long)n);
                for (size_t i = 0; i < n; i++)
                    if (std::isnan(offsets[3 * i + 1]) != std::isnan(probes[i].position.w) || probes[i].normal.z != 1.0)
                        return fail("position of a probe", (long)n, (long)i);
                if (rt_debug_probe_positions(&g, nullptr, probes.data()) != RT_OK || probes[n - 1].position.w != 1.0) return fail("positions, no offsets");
            }
    // argument errors, the outputs untouched
    rt_probe_grid g = make_grid(1, 1, 1, 0);
    rt_probe_relocate_params P = make_params(0);
    rt_ray r;
    rt_hit h;
    std::memset(&r, 0, sizeof r);
    std::memset(&h, 0, sizeof h);
    r.direction.z = 1;
    double o[3] = {-7, -7, -7};
    rt_probe_relocation rec;
    std::memset(&rec, 0x55, sizeof rec);
    rt_probe_relocate_params bad[11];
    for (rt_probe_relocate_params& b : bad) b = P;
    bad[0].back_share = -0.1, bad[1].back_share = 1.0, bad[2].back_share = nan_, bad[3].min_front = 0, bad[4].min_front = inf, bad[5].min_front = nan_;
    bad[6].max_offset = 0, bad[7].max_offset = 0.5, bad[8].max_offset = nan_, bad[9].flags = 2, bad[10].reserved = 1;
    for (const rt_probe_relocate_params& b : bad)
        if (rt_debug_probe_relocate(&g, &b, &r, &h, 1, o, &rec) != RT_ERR_ARG) return fail("params rules", (long)(&b - bad));
    rt_probe_grid badg = g;
    badg.step[2] = 0;
    rt_surfel out;
    std::memset(&out, 0x55, sizeof out);
    if (rt_debug_probe_relocate(&badg, &P, &r, &h, 1, o, &rec) != RT_ERR_ARG || rt_debug_probe_relocate(nullptr, &P, &r, &h, 1, o, &rec) != RT_ERR_ARG ||
        rt_debug_probe_relocate(&g, nullptr, &r, &h, 1, o, &rec) != RT_ERR_ARG || rt_debug_probe_relocate(&g, &P, nullptr, &h, 1, o, &rec) != RT_ERR_ARG ||
        rt_debug_probe_relocate(&g, &P, &r, nullptr, 1, o, &rec) != RT_ERR_ARG || rt_debug_probe_relocate(&g, &P, &r, &h, 0, o, &rec) != RT_ERR_ARG ||
        rt_debug_probe_relocate(&g, &P, &r, &h, (1 << 19) + 1, o, &rec) != RT_ERR_ARG || rt_debug_probe_relocate(&g, &P, &r, &h, 1, nullptr, &rec) != RT_ERR_ARG ||
        rt_debug_probe_relocate(&g, &P, &r, &h, 1, o, nullptr) != RT_ERR_ARG || rt_debug_probe_positions(&badg, o, &out) != RT_ERR_ARG ||
        rt_debug_probe_positions(nullptr, o, &out) != RT_ERR_ARG || rt_debug_probe_positions(&g, o, nullptr) != RT_ERR_ARG)
        return fail("relocate arguments");
    if (o[0] != -7 || o[2] != -7 || rec.state != 0x55555555u || rec.reserved != 0x55555555 || out.normal.w == 0.0) return fail("outputs touched");
    std::printf("ok relocate\n");
    return 0;
}

static int check_shade()
{
    const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {1, 3, 1}};
    for (const int* dm : shapes)
        for (int placed = 0; placed < 3; placed++) // both arrays, offsets only, state only
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)200}) {
                uint32_t s = 43u + (uint32_t)n + (uint32_t)dm[1] * 7u + (uint32_t)placed;
                const rt_probe_grid g = make_grid(dm[0], dm[1], dm[2], RT_PROBE_GRID_VISIBILITY), g0 = make_grid(dm[0], dm[1], dm[2], 0);
                rt_probe_depth_params P;
                std::memset(&P, 0, sizeof P);
                P.d_max = 1.5, P.var_floor = 1e-3, P.sharpness = 5, P.flags = RT_PROBE_DEPTH_WRAP;
                const size_t np = (size_t)dm[0] * dm[1] * dm[2];
                std::vector<rt_surfel> pts((size_t)n);
                for (size_t i = 0; i < pts.size(); i++) {
                    double p[3], nrm[3];
                    for (int a = 0; a < 3; a++) {
                        const double span = g.dims[a] > 1 ? (g.dims[a] - 1) * g.step[a] : g.step[a];
                        p[a] = g.origin[a] - 0.4 * span + unit(s) * 1.8 * span;
                        if (i % 4 == 1) p[a] = g.origin[a] + (double)(lcg(s) % (uint32_t)g.dims[a]) * g.step[a]; // on a grid position
                        nrm[a] = (unit(s) - 0.5) * 6;
                    }
                    pts[i].position = {p[0], p[1], p[2], 1};
                    pts[i].normal = {nrm[0], nrm[1], nrm[2], 0};
                    if (i % 50 == 7) pts[i].position.y = nan_;
                    if (i % 50 == 14) pts[i].normal = {0, 0, 0, 0};
                }
                std::vector<double> L(np * 27), D(np * 128), offsets(np * 3);
                std::vector<uint32_t> state(np);
                for (double& v : L) v = unit(s) * 2 - 0.5;
                for (size_t j = 0; j < np * 64; j++) {
                    const double mu = 0.1 + unit(s) * 1.6;
                    D[2 * j] = j % 7 == 2 ? nan_ : mu;
                    D[2 * j + 1] = j % 7 == 2 ? nan_ : mu * mu + unit(s) * 0.2 - 0.01;
                }
                for (size_t i = 0; i < np; i++) {
                    for (int a = 0; a < 3; a++) offsets[3 * i + a] = (unit(s) - 0.5) * 0.5 * g.step[a];
                    state[i] = i % 5 == 3 ? RT_PROBE_INSIDE | RT_PROBE_IDLE : i % 5 == 1 ? RT_PROBE_IDLE : 0u;
                }
                if (np > 1) offsets[3 * (np - 1)] = inf;
                const double* po = placed == 2 ? nullptr : offsets.data();
                const uint32_t* ps = placed == 1 ? nullptr : state.data();
                std::vector<rt_ray> rays((size_t)n * 8);
                std::vector<double> t_max((size_t)n * 8, -7.0);
                std::vector<uint8_t> occ((size_t)n * 8);
                for (uint8_t& b : occ) b = lcg(s) % 5u == 0;
                if (rt_debug_probe_segments_placed(&g, po, ps, n ? pts.data() : nullptr, n, n ? rays.data() : nullptr, n ? t_max.data() : nullptr) != RT_OK)
                    return fail("rt_debug_probe_segments_placed", (long)n, placed);
                for (size_t j = 0; j < (size_t)n * 8; j++)
                    if (!(t_max[j] >= 0.0) || (t_max[j] == 0.0) != (rays[j].origin.w == 0.0)) return fail("segment", (long)n, (long)j);
                std::vector<rt_color> E((size_t)n, rt_color{-7, -7, -7});
                std::vector<double> w((size_t)n, -7.0);
                for (int pass = 0; pass < 4; pass++) { // blend and depth blend, with and without a weight array
                    const int rc = pass < 2 ? rt_debug_shade_probes_placed(&g, po, ps, n ? L.data() : nullptr, n ? pts.data() : nullptr, n,
                                                                           n ? occ.data() : nullptr, n ? E.data() : nullptr,
                                                                           pass & 1 || !n ? nullptr : w.data())
                                            : rt_debug_shade_probes_depth_placed(&g0, po, ps, &P, n ? L.data() : nullptr, n ? D.data() : nullptr,
                                                                                 n ? pts.data() : nullptr, n, n ? E.data() : nullptr,
                                                                                 pass & 1 || !n ? nullptr : w.data());
                    if (rc != RT_OK) return fail("placed shade", (long)n, pass);
                    for (size_t i = 0; i < (size_t)n; i++) {
                        if (!(w[i] >= 0.0 && w[i] <= 1.2 * (1.0 + 1e-15))) return fail("weight range", (long)n, (long)i);
                        if (!std::isfinite(E[i].r) || !std::isfinite(E[i].g) || !std::isfinite(E[i].b)) return fail("irradiance finite", (long)n, (long)i);
                        if (w[i] == 0.0 && (E[i].r != 0 || E[i].g != 0 || E[i].b != 0)) return fail("zeros of a point without a probe", (long)n, (long)i);
                    }
                }
            }
    std::printf("ok shade\n");
    return 0;
}

int main()
{
    if (check_relocate()) return 1;
    if (check_shade()) return 1;
    std::printf("probe_relocate_host_check: ok\n");
    return 0;
}
