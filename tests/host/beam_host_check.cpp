// beam_host_check.cpp -- rt_debug_beam_rays and rt_camera_beams under AddressSanitizer and
// UndefinedBehaviorSanitizer (`make -C raytracercore_amd/csrc beam_host_check_asan`;
// tests/test_render_beams_host.py runs it).  Every array is allocated at its exact size so that a read
// or write past it is reported: the twin over n = 1, 63, 1025 and 5000 beams at 1 and 7 samples, with and
// without uv_out, among them invalid and degenerate beams; rt_camera_beams over the tiles 1 x 1, 16 x 8
// and the whole 37 x 19 frame for both camera kinds; the argument errors.  No device is touched.
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
static double unit(uint32_t& s) { return (double)(lcg(s) >> 8) * (1.0 / 16777216.0) - 0.5; }

static int twin()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)1025, (int64_t)5000})
        for (int32_t spp : {1, 7})
            for (bool with_uv : {true, false}) {
                uint32_t s = 17u + (uint32_t)n;
                std::vector<rt_beam> beams((size_t)n);
                for (rt_beam& b : beams) {
                    b.origin = {unit(s) * 8, unit(s) * 8, unit(s) * 8, 1};
                    b.direction = {unit(s), unit(s), unit(s) + 0.75, 0};
                    b.origin_du = {unit(s) * .1, unit(s) * .1, unit(s) * .1, 0};
                    b.origin_dv = {unit(s) * .1, unit(s) * .1, unit(s) * .1, 0};
                    b.direction_du = {unit(s) * .02, unit(s) * .02, unit(s) * .02, 0};
                    b.direction_dv = {unit(s) * .02, unit(s) * .02, unit(s) * .02, 0};
                }
                const size_t bad = (size_t)(n / 2), zero = (size_t)(n - 1);
                if (n > 1) {
                    beams[bad].origin_dv.w = nan; // invalid: an ignored component that is not finite
                    beams[zero].direction = beams[zero].direction_du = beams[zero].direction_dv = {0, 0, 0, 0};
                }
                std::vector<rt_ray> rays((size_t)n * spp);
                std::vector<double> uv(with_uv ? (size_t)n * spp * 2 : 0);
                if (rt_debug_beam_rays(beams.data(), n, spp, 99, 5, 1ull << 40, rays.data(), with_uv ? uv.data() : nullptr) != RT_OK)
                    return fail("rt_debug_beam_rays", (long)n, spp);
                for (size_t i = 0; i < (size_t)n; i++)
                    for (int k = 0; k < spp; k++) {
                        const rt_ray& r = rays[i * spp + k];
                        const double len = std::sqrt(r.direction.x * r.direction.x + r.direction.y * r.direction.y +
                                                     r.direction.z * r.direction.z);
                        const bool miss = n > 1 && (i == bad || i == zero);
                        if (miss ? (len != 0.0 || r.origin.w != 0.0) : (std::fabs(len - 1.0) > 1e-6 || r.origin.w != 1.0))
                            return fail("ray", (long)i, k);
                        if (with_uv && !(uv[2 * (i * spp + k)] >= 0.0 && uv[2 * (i * spp + k) + 1] < 1.0)) return fail("uv", (long)i, k);
                    }
            }
    rt_beam b;
    std::memset(&b, 0, sizeof b);
    rt_ray r;
    if (rt_debug_beam_rays(&b, -1, 1, 0, 0, 0, &r, nullptr) != RT_ERR_ARG || rt_debug_beam_rays(&b, 1, 0, 0, 0, 0, &r, nullptr) != RT_ERR_ARG ||
        rt_debug_beam_rays(nullptr, 1, 1, 0, 0, 0, &r, nullptr) != RT_ERR_ARG || rt_debug_beam_rays(&b, 1, 1, 0, 0, 0, nullptr, nullptr) != RT_ERR_ARG ||
        rt_debug_beam_rays(nullptr, 0, 1, 0, 0, 0, nullptr, nullptr) != RT_OK)
        return fail("twin arguments");
    std::printf("ok twin\n");
    return 0;
}

static int cameras()
{
    const int W = 37, H = 19;
    for (int kind : {(int)RT_CAMERA_FRUSTUM, (int)RT_CAMERA_ORTHO}) {
        rt_camera cam;
        std::memset(&cam, 0, sizeof cam);
        cam.kind = kind;
        cam.position = {0.25, -0.5, 0, 1};
        cam.look_at = {0.5, 0.25, 4, 1};
        cam.up = {0, 1, 0, 0};
        cam.fov_y = 1.2;
        cam.size_mult = 3.0;
        const int tiles[][4] = {{36, 18, 1, 1}, {5, 3, 16, 8}, {0, 0, W, H}};
        for (const auto& t : tiles) {
            const size_t n = (size_t)t[2] * t[3];
            std::vector<rt_beam> beams(n);
            std::vector<rt_ray> rays(n);
            if (rt_camera_beams(&cam, W, H, t[0], t[1], t[2], t[3], beams.data()) != RT_OK) return fail("rt_camera_beams", kind, t[2]);
            if (rt_camera_rays(&cam, W, H, t[0], t[1], t[2], t[3], rays.data()) != RT_OK) return fail("rt_camera_rays", kind, t[2]);
            for (size_t i = 0; i < n; i++) { // at (0, 0) the beam is the pixel's ray
                const rt_vec4d d = beams[i].direction;
                const double len = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
                if (std::fabs(d.x / len - rays[i].direction.x) > 1e-14 || std::fabs(d.y / len - rays[i].direction.y) > 1e-14 ||
                    std::fabs(d.z / len - rays[i].direction.z) > 1e-14 || beams[i].origin.x != rays[i].origin.x)
                    return fail("beam at (0, 0)", kind, (long)i);
            }
            // and it feeds the twin
            std::vector<rt_ray> out(n * 2);
            if (rt_debug_beam_rays(beams.data(), (int64_t)n, 2, 1, 0, 0, out.data(), nullptr) != RT_OK) return fail("twin on camera beams");
        }
        rt_beam one;
        if (rt_camera_beams(&cam, W, H, 30, 0, 8, 1, &one) != RT_ERR_ARG || rt_camera_beams(&cam, W, H, 0, 0, 0, 1, &one) != RT_ERR_ARG ||
            rt_camera_beams(nullptr, W, H, 0, 0, 1, 1, &one) != RT_ERR_ARG || rt_camera_beams(&cam, W, H, 0, 0, 1, 1, nullptr) != RT_ERR_ARG)
            return fail("camera arguments", kind);
    }
    std::printf("ok cameras\n");
    return 0;
}

int main()
{
    if (twin()) return 1;
    if (cameras()) return 1;
    std::printf("beam_host_check: ok\n");
    return 0;
}
