// probe_list_host_check.cpp -- rt_debug_probe_moments, rt_debug_probe_error and rt_debug_probe_select under
// AddressSanitizer and UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc probe_list_host_check_asan`;
// tests/test_probe_list_host.py runs it).  Every array is allocated at its exact size so that a read or write
// past it is reported: the moments over n = 0, 1, 5 and 129 probes at spp = 1, 7 and 70, with hits, misses and
// all-zero rays, checked against a restatement written here; the rule over the same accumulators with cap 0,
// below and at the count; the argument errors.  No device is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rtcore.h"

static int fail(const char* what, long a = 0, long b = 0)
{
    std::printf("FAILED %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t& s) { return (double)(lcg(s) >> 8) * (1.0 / 16777216.0) - 0.5; }

static const double K0 = 0.28209479177387814, K1 = 0.48860251190291992, PI = 3.141592653589793;

// the formulas of rtcore.h, "adaptive light probes" (this file is built with -ffp-contract=off)
static bool active(const rt_probe_select_params& P, const rt_probe_sh& c, uint32_t ns, uint32_t nm, const rt_probe_moments& m,
                   double* se_out, double* level_out)
{
    const uint64_t N = (uint64_t)ns + nm;
    *se_out = *level_out = NAN;
    bool ok = true;
    if (N >= 2) {
        const double n = (double)N;
        const double A = (0.299 * P.ambient.r + 0.587 * P.ambient.g) + 0.114 * P.ambient.b, AA = A * A;
        double S[4], v[4];
        for (int l = 0; l < 4; l++) {
            S[l] = ((0.299 * c.c[l][0] + 0.587 * c.c[l][1]) + 0.114 * c.c[l][2]) + A * c.c[l][3];
            const double T = m.m[l][0] + AA * m.m[l][1];
            const double num = T - (S[l] * S[l]) / n;
            const double d = num / (n - 1.0);
            v[l] = num > (n * 0x1p-49) * T ? d : 0;
            ok = ok && !std::isnan(d);
        }
        const double a0 = PI * K0, a1 = 2.0943951023931953 * K1, p4 = 4.0 * PI;
        *level_out = ((p4 * a0) * S[0]) / n;
        *se_out = p4 * std::sqrt(((a0 * a0) * v[0] + (a1 * a1) * ((v[1] + v[2]) + v[3])) / n);
    }
    if (N < P.min_samples) return true;
    if (N >= P.max_samples) return false;
    if (N < 2) return true;
    if (!ok) return false;
    const double lv = *level_out > P.irr_floor ? *level_out : P.irr_floor;
    return *se_out > P.rel_tol * lv;
}

static bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof a) == 0; }

static int check_all()
{
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)129})
        for (int32_t spp : {1, 7, 70}) {
            uint32_t s = 41u + (uint32_t)n * 3u + (uint32_t)spp;
            const size_t total = (size_t)n * (size_t)spp;
            std::vector<rt_ray> rays(total);
            std::vector<float> rgb(total * 3);
            std::vector<uint8_t> miss(total);
            for (size_t at = 0; at < total; at++) {
                rays[at].origin = {unit(s), unit(s), unit(s), 1};
                rays[at].direction = {(double)(float)unit(s), (double)(float)unit(s), (double)(float)(unit(s) + 0.75), 0};
                if (lcg(s) % 11u == 0) std::memset(&rays[at], 0, sizeof(rt_ray)); // an invalid probe's sample
                for (int j = 0; j < 3; j++) rgb[3 * at + j] = (float)(unit(s) + 0.5);
                miss[at] = (uint8_t)(lcg(s) % 3u == 0 ? 1 + lcg(s) % 200u : 0);
            }
            std::vector<rt_probe_moments> mom((size_t)n), want((size_t)n);
            std::vector<rt_probe_sh> sh((size_t)n);
            std::vector<uint32_t> ns((size_t)n, 0u), nm((size_t)n, 0u);
            for (size_t i = 0; i < (size_t)n; i++)
                for (int l = 0; l < 4; l++)
                    for (int j = 0; j < 2; j++) mom[i].m[l][j] = want[i].m[l][j] = unit(s) + 0.5; // added to what is there
            if (n) std::memset(sh.data(), 0, sh.size() * sizeof(rt_probe_sh));
            if (rt_debug_probe_moments(n ? rays.data() : nullptr, n ? rgb.data() : nullptr, n ? miss.data() : nullptr, n, spp,
                                       n ? mom.data() : nullptr) != RT_OK)
                return fail("rt_debug_probe_moments", (long)n, spp);
            if (rt_debug_probe_fold(n ? rays.data() : nullptr, n ? rgb.data() : nullptr, n ? miss.data() : nullptr, n, spp,
                                    n ? sh.data() : nullptr, n ? ns.data() : nullptr, n ? nm.data() : nullptr) != RT_OK)
                return fail("rt_debug_probe_fold", (long)n, spp);
            for (size_t i = 0; i < (size_t)n; i++) {
                for (size_t at = i * spp; at < (i + 1) * (size_t)spp; at++) {
                    const rt_vec4d d = rays[at].direction;
                    if (d.x == 0 && d.y == 0 && d.z == 0) continue;
                    const double Y[4] = {K0, K1 * d.y, K1 * d.z, K1 * d.x};
                    if (miss[at]) {
                        for (int l = 0; l < 4; l++) want[i].m[l][1] = want[i].m[l][1] + Y[l] * Y[l];
                    } else {
                        const double y = (0.299 * (double)rgb[3 * at] + 0.587 * (double)rgb[3 * at + 1]) + 0.114 * (double)rgb[3 * at + 2];
                        for (int l = 0; l < 4; l++) {
                            const double x = y * Y[l];
                            want[i].m[l][0] = want[i].m[l][0] + x * x;
                        }
                    }
                }
                if (std::memcmp(&want[i], &mom[i], sizeof(rt_probe_moments)) != 0) return fail("moments bits", (long)n, (long)i);
            }
            // the rule over these accumulators
            const rt_probe_select_params P = {0.05, 1e-3, {0.5, 0.25, 1.0}, 2u, 60u};
            std::vector<double> se((size_t)n, -7.0), level((size_t)n, -7.0);
            if (rt_debug_probe_error(&P, n ? sh.data() : nullptr, n ? ns.data() : nullptr, n ? nm.data() : nullptr,
                                     n ? mom.data() : nullptr, n, n ? se.data() : nullptr, n ? level.data() : nullptr) != RT_OK)
                return fail("rt_debug_probe_error", (long)n, spp);
            std::vector<uint32_t> expect;
            for (size_t i = 0; i < (size_t)n; i++) {
                double wse, wlevel;
                if (active(P, sh[i], ns[i], nm[i], mom[i], &wse, &wlevel)) expect.push_back((uint32_t)i);
                if (!same(wse, se[i]) || !same(wlevel, level[i])) return fail("error bits", (long)n, (long)i);
            }
            if (n == 0) continue; // (n_records <= 0 is an argument error: below)
            for (uint32_t cap : {0u, (uint32_t)(expect.size() / 2), (uint32_t)expect.size()}) {
                std::vector<uint32_t> list(cap, 0xFFFFFFFFu);
                const int64_t k = rt_debug_probe_select(&P, sh.data(), ns.data(), nm.data(), mom.data(), n, cap ? list.data() : nullptr, cap);
                if (k != (int64_t)expect.size()) return fail("select count", (long)n, (long)k);
                if (cap && std::memcmp(list.data(), expect.data(), cap * sizeof(uint32_t)) != 0) return fail("select list", (long)n, (long)cap);
            }
        }
    std::printf("ok moments, error, select\n");
    return 0;
}

static int check_arguments()
{
    rt_ray r;
    std::memset(&r, 0, sizeof r);
    float c[3] = {0, 0, 0};
    uint8_t m = 0;
    rt_probe_moments mom;
    std::memset(&mom, 0, sizeof mom);
    rt_probe_sh sh;
    std::memset(&sh, 0, sizeof sh);
    uint32_t a = 0, b = 0, e = 0;
    double se = 0, level = 0;
    if (rt_debug_probe_moments(&r, c, &m, -1, 1, &mom) != RT_ERR_ARG || rt_debug_probe_moments(&r, c, &m, 1, 0, &mom) != RT_ERR_ARG ||
        rt_debug_probe_moments(nullptr, c, &m, 1, 1, &mom) != RT_ERR_ARG || rt_debug_probe_moments(&r, nullptr, &m, 1, 1, &mom) != RT_ERR_ARG ||
        rt_debug_probe_moments(&r, c, nullptr, 1, 1, &mom) != RT_ERR_ARG || rt_debug_probe_moments(&r, c, &m, 1, 1, nullptr) != RT_ERR_ARG ||
        rt_debug_probe_moments(nullptr, nullptr, nullptr, 0, 1, nullptr) != RT_OK)
        return fail("moments arguments");
    rt_probe_select_params P = {0.1, 1e-3, {0, 0, 0}, 1u, 8u};
    if (rt_debug_probe_error(nullptr, &sh, &a, &b, &mom, 1, &se, &level) != RT_ERR_ARG ||
        rt_debug_probe_error(&P, &sh, &a, &b, &mom, -1, &se, &level) != RT_ERR_ARG ||
        rt_debug_probe_error(&P, nullptr, &a, &b, &mom, 1, &se, &level) != RT_ERR_ARG ||
        rt_debug_probe_error(&P, &sh, &a, &b, &mom, 1, nullptr, &level) != RT_ERR_ARG ||
        rt_debug_probe_error(&P, &sh, &a, &b, &mom, 1, &se, nullptr) != RT_ERR_ARG ||
        rt_debug_probe_error(&P, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != RT_OK)
        return fail("error arguments");
    rt_probe_select_params neg = P, nan_tol = P, zero_floor = P, nan_floor = P;
    neg.rel_tol = -1;
    nan_tol.rel_tol = NAN;
    zero_floor.irr_floor = 0;
    nan_floor.irr_floor = NAN;
    if (rt_debug_probe_select(nullptr, &sh, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG || rt_debug_probe_select(&P, nullptr, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&P, &sh, nullptr, &b, &mom, 1, &e, 1) != RT_ERR_ARG || rt_debug_probe_select(&P, &sh, &a, nullptr, &mom, 1, &e, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&P, &sh, &a, &b, nullptr, 1, &e, 1) != RT_ERR_ARG || rt_debug_probe_select(&P, &sh, &a, &b, &mom, 1, nullptr, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&P, &sh, &a, &b, &mom, 0, &e, 1) != RT_ERR_ARG || rt_debug_probe_select(&P, &sh, &a, &b, &mom, (int64_t)1 << 32, &e, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&neg, &sh, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG || rt_debug_probe_select(&nan_tol, &sh, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&zero_floor, &sh, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG ||
        rt_debug_probe_select(&nan_floor, &sh, &a, &b, &mom, 1, &e, 1) != RT_ERR_ARG)
        return fail("select arguments");
    if (rt_debug_probe_select(&P, &sh, &a, &b, &mom, 1, nullptr, 0) != 1) return fail("select without a list"); // N = 0 < min
    std::printf("ok arguments\n");
    return 0;
}

int main()
{
    if (check_all()) return 1;
    if (check_arguments()) return 1;
    std::printf("probe_list_host_check: ok\n");
    return 0;
}
