// probe_host_check.cpp -- rt_debug_sh_basis and rt_debug_probe_fold under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc probe_host_check_asan`;
// tests/test_render_probes_host.py runs it).  Every array is allocated at its exact size so that a read or
// write past it is reported: the basis over n = 0, 1, 63 and 1025 directions; the fold over n = 0, 1, 5 and
// 129 probes at spp = 1, 7 and 70, with hits, misses and all-zero rays, checked against a restatement
// written here; the argument errors.  No device is touched.
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

// the formulas of rtcore.h, "light probes" (this file is built with -ffp-contract=off)
static void basis(double x, double y, double z, double* Y)
{
    const double K0 = 0.28209479177387814, K1 = 0.48860251190291992, K2 = 1.0925484305920792;
    const double K3 = 0.31539156525252005, K4 = 0.54627421529603959;
    Y[0] = K0;
    Y[1] = K1 * y;
    Y[2] = K1 * z;
    Y[3] = K1 * x;
    Y[4] = (K2 * x) * y;
    Y[5] = (K2 * y) * z;
    Y[6] = K3 * ((3 * z) * z - 1);
    Y[7] = (K2 * x) * z;
    Y[8] = K4 * (x * x - y * y);
}

static int check_basis()
{
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)63, (int64_t)1025}) {
        uint32_t s = 5u + (uint32_t)n;
        std::vector<double> dirs((size_t)n * 3), y((size_t)n * 9, -7.0);
        for (double& v : dirs) v = unit(s) * 2;
        if (rt_debug_sh_basis(n ? dirs.data() : nullptr, n, n ? y.data() : nullptr) != RT_OK) return fail("rt_debug_sh_basis", (long)n);
        for (size_t i = 0; i < (size_t)n; i++) {
            double want[9];
            basis(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], want);
            if (std::memcmp(want, &y[9 * i], sizeof want) != 0) return fail("basis bits", (long)n, (long)i);
        }
    }
    double d[3] = {0, 0, 1}, y[9];
    if (rt_debug_sh_basis(d, -1, y) != RT_ERR_ARG || rt_debug_sh_basis(nullptr, 1, y) != RT_ERR_ARG ||
        rt_debug_sh_basis(d, 1, nullptr) != RT_ERR_ARG)
        return fail("basis arguments");
    std::printf("ok basis\n");
    return 0;
}

static int check_fold()
{
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)129})
        for (int32_t spp : {1, 7, 70}) {
            uint32_t s = 23u + (uint32_t)n * 3u + (uint32_t)spp;
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
            std::vector<rt_probe_sh> sh((size_t)n), want((size_t)n);
            std::vector<uint32_t> ns((size_t)n, 3u), nm((size_t)n, 4u), wns((size_t)n, 3u), wnm((size_t)n, 4u);
            for (size_t i = 0; i < (size_t)n; i++)
                for (int l = 0; l < 9; l++)
                    for (int j = 0; j < 4; j++) sh[i].c[l][j] = want[i].c[l][j] = unit(s) * 4; // added to what is there
            if (rt_debug_probe_fold(n ? rays.data() : nullptr, n ? rgb.data() : nullptr, n ? miss.data() : nullptr, n, spp,
                                    n ? sh.data() : nullptr, n ? ns.data() : nullptr, n ? nm.data() : nullptr) != RT_OK)
                return fail("rt_debug_probe_fold", (long)n, spp);
            for (size_t i = 0; i < (size_t)n; i++) {
                for (size_t at = i * spp; at < (i + 1) * (size_t)spp; at++) {
                    const rt_vec4d d = rays[at].direction;
                    if (d.x == 0 && d.y == 0 && d.z == 0) {
                        wnm[i]++;
                        continue;
                    }
                    double Y[9];
                    basis(d.x, d.y, d.z, Y);
                    if (miss[at]) {
                        wnm[i]++;
                        for (int l = 0; l < 9; l++) want[i].c[l][3] = want[i].c[l][3] + Y[l];
                    } else {
                        wns[i]++;
                        for (int l = 0; l < 9; l++)
                            for (int j = 0; j < 3; j++) want[i].c[l][j] = want[i].c[l][j] + ((double)rgb[3 * at + j] * Y[l]);
                    }
                }
                if (std::memcmp(&want[i], &sh[i], sizeof(rt_probe_sh)) != 0) return fail("fold bits", (long)n, (long)i);
                if (ns[i] != wns[i] || nm[i] != wnm[i] || ns[i] + nm[i] != 7u + (uint32_t)spp) return fail("fold counts", (long)n, (long)i);
            }
        }
    rt_ray r;
    std::memset(&r, 0, sizeof r);
    float c[3] = {0, 0, 0};
    uint8_t m = 0;
    rt_probe_sh sh;
    std::memset(&sh, 0, sizeof sh);
    uint32_t a = 0, b = 0;
    if (rt_debug_probe_fold(&r, c, &m, -1, 1, &sh, &a, &b) != RT_ERR_ARG || rt_debug_probe_fold(&r, c, &m, 1, 0, &sh, &a, &b) != RT_ERR_ARG ||
        rt_debug_probe_fold(nullptr, c, &m, 1, 1, &sh, &a, &b) != RT_ERR_ARG || rt_debug_probe_fold(&r, nullptr, &m, 1, 1, &sh, &a, &b) != RT_ERR_ARG ||
        rt_debug_probe_fold(&r, c, nullptr, 1, 1, &sh, &a, &b) != RT_ERR_ARG || rt_debug_probe_fold(&r, c, &m, 1, 1, nullptr, &a, &b) != RT_ERR_ARG ||
        rt_debug_probe_fold(&r, c, &m, 1, 1, &sh, nullptr, &b) != RT_ERR_ARG || rt_debug_probe_fold(&r, c, &m, 1, 1, &sh, &a, nullptr) != RT_ERR_ARG ||
        rt_debug_probe_fold(nullptr, nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr) != RT_OK || a != 0 || b != 0)
        return fail("fold arguments");
    std::printf("ok fold\n");
    return 0;
}

int main()
{
    if (check_basis()) return 1;
    if (check_fold()) return 1;
    std::printf("probe_host_check: ok\n");
    return 0;
}
