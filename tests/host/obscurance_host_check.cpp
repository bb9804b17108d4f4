// obscurance_host_check.cpp -- rt_debug_obscurance_fold, rt_debug_obscurance_select and rt_debug_obscurance_error
// under AddressSanitizer and UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc
// obscurance_host_check_asan`; tests/test_obscurance_host.py runs it).  Every array is allocated at its exact
// size so that a read or write past it is reported; what must hold whatever the numbers are is checked here, the
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

static rt_obscurance_params make_params(double radius, int power)
{
    rt_obscurance_params p;
    std::memset(&p, 0, sizeof p);
    p.radius = radius;
    p.power = power;
    return p;
}

static int check_fold()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int power : {0, 1, 2, 8})
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)7})
            for (int32_t spp : {1, 5, 64, 65, 130}) {
                uint32_t s = 17u + (uint32_t)n * 3u + (uint32_t)spp + (uint32_t)power;
                const rt_obscurance_params P = make_params(1.5, power);
                const size_t m = (size_t)n * (size_t)spp;
                std::vector<rt_ray> rays(m);
                std::vector<rt_hit> hits(m);
                std::vector<uint32_t> want_hits((size_t)n, 0u), valid((size_t)n, 0u);
                for (size_t j = 0; j < m; j++) {
                    std::memset(&rays[j], 0, sizeof(rt_ray));
                    std::memset(&hits[j], 0, sizeof(rt_hit));
                    double d[3] = {unit(s) - 0.5, unit(s) - 0.5, unit(s) - 0.5};
                    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                    const bool zero = j % 11 == 3 || !(len > 0);
                    rays[j].direction = zero ? rt_vec4d{0, 0, 0, 0} : rt_vec4d{(double)(float)(d[0] / len), (double)(float)(d[1] / len), (double)(float)(d[2] / len), 0};
                    hits[j].prim_id = j % 4 == 1 ? -1 : (int32_t)(j % 9);
                    hits[j].distance = hits[j].prim_id < 0 ? 0.0 : j % 13 == 5 ? nan : j % 17 == 2 ? P.radius : unit(s) * 3.0; // (half of them past the radius)
                    if (!zero) valid[j / (size_t)spp]++;
                    if (!zero && hits[j].prim_id >= 0 && hits[j].distance < P.radius) want_hits[j / (size_t)spp]++;
                }
                std::vector<rt_obscurance> acc((size_t)n);
                if (n) std::memset(acc.data(), 0, acc.size() * sizeof(rt_obscurance));
                if (rt_debug_obscurance_fold(&P, n ? rays.data() : nullptr, n ? hits.data() : nullptr, n, spp, n ? acc.data() : nullptr) != RT_OK)
                    return fail("rt_debug_obscurance_fold", (long)n, spp);
                for (size_t i = 0; i < (size_t)n; i++) {
                    const rt_obscurance& a = acc[i];
                    if (a.samples != (uint32_t)spp || a.hits != want_hits[i]) return fail("counts of an entry", (long)n, (long)i);
                    // weights lie in [0, 1]: 0 <= o2 <= o <= hits, and the bent normal is no longer than the valid samples' (1 - w)
                    if (!(a.o >= 0 && a.o2 >= 0 && a.o2 <= a.o * (1 + 1e-12) && a.o <= (double)a.hits * (1 + 1e-12)))
                        return fail("sums of an entry", (long)n, (long)i);
                    if (power == 0 && (a.o != (double)a.hits || a.o2 != a.o)) return fail("power 0 counts hits", (long)n, (long)i);
                    const double len = std::sqrt(a.bent[0] * a.bent[0] + a.bent[1] * a.bent[1] + a.bent[2] * a.bent[2]);
                    if (!(len <= ((double)valid[i] - a.o) * (1 + 1e-6) + 1e-12)) return fail("bent normal's length", (long)n, (long)i);
                }
                // the rule over what the fold gave, at every cap
                rt_obscurance_select_params S = {0.05, 2, 100};
                std::vector<double> se((size_t)n, -7.0), mean((size_t)n, -7.0);
                if (rt_debug_obscurance_error(&S, n ? acc.data() : nullptr, n, n ? se.data() : nullptr, n ? mean.data() : nullptr) != RT_OK)
                    return fail("rt_debug_obscurance_error", (long)n, spp);
                for (size_t i = 0; i < (size_t)n; i++)
                    if (spp < 2 ? !(std::isnan(se[i]) && std::isnan(mean[i])) : !(se[i] >= 0 && se[i] <= 1 && mean[i] >= 0 && mean[i] <= 1))
                        return fail("error range", (long)n, (long)i);
                if (n == 0) continue;
                for (uint32_t cap : {0u, 1u, (uint32_t)n}) {
                    std::vector<uint32_t> list(cap, 0xffffffffu);
                    const int64_t k = rt_debug_obscurance_select(&S, acc.data(), n, cap ? list.data() : nullptr, cap);
                    if (k < 0 || k > n) return fail("rt_debug_obscurance_select", (long)n, (long)k);
                    for (uint32_t j = 0; j < cap; j++) {
                        if ((int64_t)j < k ? list[j] >= (uint32_t)n || (j > 0 && list[j] <= list[j - 1]) : list[j] != 0xffffffffu)
                            return fail("list", (long)n, j);
                    }
                    if (spp < 2 && k != n) return fail("below min_samples every entry is active", (long)n, (long)k);
                    if (spp >= 100 && k != 0) return fail("at max_samples no entry is active", (long)n, (long)k);
                }
            }
    std::printf("ok fold, error and select\n");
    return 0;
}

static int check_arguments()
{
    rt_obscurance_params P = make_params(1.5, 1);
    rt_ray r;
    rt_hit h;
    std::memset(&r, 0, sizeof r);
    std::memset(&h, 0, sizeof h);
    r.direction.z = 1;
    rt_obscurance a = {-7, -7, {-7, -7, -7}, 7, 7};
    rt_obscurance_params bad[8];
    for (rt_obscurance_params& b : bad) b = P;
    bad[0].radius = 0, bad[1].radius = std::numeric_limits<double>::infinity(), bad[2].radius = std::numeric_limits<double>::quiet_NaN();
    bad[3].radius = -1, bad[4].power = -1, bad[5].power = 9, bad[6].reserved[0] = 1, bad[7].reserved[2] = 1;
    for (const rt_obscurance_params& b : bad)
        if (rt_debug_obscurance_fold(&b, &r, &h, 1, 1, &a) != RT_ERR_ARG) return fail("params rules", (long)(&b - bad));
    if (rt_debug_obscurance_fold(nullptr, &r, &h, 1, 1, &a) != RT_ERR_ARG || rt_debug_obscurance_fold(&P, nullptr, &h, 1, 1, &a) != RT_ERR_ARG ||
        rt_debug_obscurance_fold(&P, &r, nullptr, 1, 1, &a) != RT_ERR_ARG || rt_debug_obscurance_fold(&P, &r, &h, 1, 1, nullptr) != RT_ERR_ARG ||
        rt_debug_obscurance_fold(&P, &r, &h, -1, 1, &a) != RT_ERR_ARG || rt_debug_obscurance_fold(&P, &r, &h, 1, 0, &a) != RT_ERR_ARG ||
        rt_debug_obscurance_fold(&P, nullptr, nullptr, 0, 1, nullptr) != RT_OK)
        return fail("fold arguments");
    rt_obscurance_select_params S = {0.05, 2, 100}, neg = {-1.0, 2, 100}, nn = {std::numeric_limits<double>::quiet_NaN(), 2, 100};
    uint32_t list[1] = {7};
    double se = -7, mean = -7;
    if (rt_debug_obscurance_select(nullptr, &a, 1, list, 1) != RT_ERR_ARG || rt_debug_obscurance_select(&S, nullptr, 1, list, 1) != RT_ERR_ARG ||
        rt_debug_obscurance_select(&S, &a, 1, nullptr, 1) != RT_ERR_ARG || rt_debug_obscurance_select(&S, &a, 0, list, 1) != RT_ERR_ARG ||
        rt_debug_obscurance_select(&S, &a, (int64_t)1 << 32, list, 1) != RT_ERR_ARG || rt_debug_obscurance_select(&neg, &a, 1, list, 1) != RT_ERR_ARG ||
        rt_debug_obscurance_select(&nn, &a, 1, list, 1) != RT_ERR_ARG || rt_debug_obscurance_select(&S, &a, 1, nullptr, 0) < 0)
        return fail("select arguments");
    if (rt_debug_obscurance_error(nullptr, &a, 1, &se, &mean) != RT_ERR_ARG || rt_debug_obscurance_error(&S, nullptr, 1, &se, &mean) != RT_ERR_ARG ||
        rt_debug_obscurance_error(&S, &a, 1, nullptr, &mean) != RT_ERR_ARG || rt_debug_obscurance_error(&S, &a, 1, &se, nullptr) != RT_ERR_ARG ||
        rt_debug_obscurance_error(&S, &a, -1, &se, &mean) != RT_ERR_ARG || rt_debug_obscurance_error(&S, nullptr, 0, nullptr, nullptr) != RT_OK)
        return fail("error arguments");
    // the device entries end in their argument checks: nothing is launched
    if (rt_obscurance_surfels_device(nullptr, RT_GATHER_COSINE, nullptr, 1, nullptr, 1, &P, 1, 0, 0, 0, nullptr, nullptr) != RT_ERR_ARG ||
        rt_obscurance_surfels_device(nullptr, 99, nullptr, 1, nullptr, 0, &P, 1, 0, 0, 0, nullptr, nullptr) != RT_ERR_ARG ||
        rt_obscurance_select_device(&neg, &a, 1, list, 1, list, nullptr) != RT_ERR_ARG ||
        rt_obscurance_select_device(&S, &a, 1, list, 1, nullptr, nullptr) != RT_ERR_ARG)
        return fail("device entry arguments");
    if (a.o != -7 || a.o2 != -7 || a.bent[2] != -7 || a.samples != 7 || a.hits != 7 || list[0] != 7 || se != -7 || mean != -7)
        return fail("outputs touched");
    std::printf("ok arguments\n");
    return 0;
}

int main()
{
    if (check_fold()) return 1;
    if (check_arguments()) return 1;
    std::printf("obscurance_host_check: ok\n");
    return 0;
}
