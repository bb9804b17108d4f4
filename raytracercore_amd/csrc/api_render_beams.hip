// api_render_beams.hip -- the C ABI's radiance queries for beams (include/rtcore.h, "radiance queries",
// rt_beam): rt_render_rays with the sample's point in a first-order footprint drawn on the device, by
// the BEAMS instances of the path kernels (kernels_path.hip, refill).  The entry points' bodies are
// rt_render_rays' (api_render_rays.hip); here are the host twin of the sample's ray (rt_beam.h, the
// kernel's own function compiled for the host) and the beams of the library's cameras.
#include "rt_scene.h"
#include "rt_beam.h"
#include "rt_refmath.h"

static_assert(sizeof(rt_beam) == kBeamRows * 16 && sizeof(rt_beam) % sizeof(rt_ray) == 0, "rt_beam: twelve 16-byte rows");

namespace {

// 2^18 beams are 48 MiB: with the records, two chunks take 112 MiB of device scratch and as much
// pinned staging (rt_render_rays' two chunks of 2^19 rays: 96 MiB each)
constexpr int64_t kBeamsChunk = 1 << 18;
constexpr RenderList kBeams = {ITEMS_BEAMS, sizeof(rt_beam), kBeamsChunk, "beams"};

rt_vec4d vec4(Vec4d a, double w) { return rt_vec4d{a.x, a.y, a.z, w}; }

} // namespace

extern "C" {

int rt_render_beams_device(rt_scene* s, const rt_beam* d_beams, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                           uint64_t stream_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                           unsigned long long* d_count, void* stream)
{
    return render_list_device(s, kBeams, "rt_render_beams_device", d_beams, n, spp, seed, sample_base, stream_base, d_sum,
                              d_samples, d_misses, d_count, stream);
}

int rt_render_beams(rt_scene* s, const rt_beam* beams, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                    uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    return render_list_host(s, kBeams, "rt_render_beams", beams, n, spp, seed, sample_base, stream_base, sum_rgb, samples,
                            misses, rays_out);
}

// The sample start of the BEAMS instances (refill), on the host: the same draws and the same function
// of rt_beam.h on the same inputs, in the kernel's order.
int rt_debug_beam_rays(const rt_beam* beams, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                       uint64_t stream_base, rt_ray* rays_out, double* uv_out)
{
    if (n < 0 || spp <= 0 || (n > 0 && (!beams || !rays_out))) {
        set_error("rt_debug_beam_rays: bad argument (null pointer, n < 0 or spp <= 0)");
        return RT_ERR_ARG;
    }
    const rt_key2 seed_key = rt_rng_seed_key(seed);
    const double2* rows = reinterpret_cast<const double2*>(beams);
    parallel_ranges((size_t)n, 1024, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const rt_key2 pkey = rt_rng_pixel_key(seed_key, stream_base + (uint64_t)i);
            for (int32_t k = 0; k < spp; k++) {
                const size_t at = i * (size_t)spp + (size_t)k;
                rt_rng rng = rt_rng_from_pixel_key(pkey, sample_base + (uint64_t)k);
                const float u = (float)rt_rng_next24(&rng) * 0x1p-24f;
                const float v = (float)rt_rng_next24(&rng) * 0x1p-24f;
                if (uv_out) {
                    uv_out[2 * at] = (double)u;
                    uv_out[2 * at + 1] = (double)v;
                }
                BeamV o, d;
                if (beam_sample(rows + (size_t)kBeamRows * i, u, v, o, d) == BEAM_RAY)
                    rays_out[at] = rt_ray{rt_vec4d{(double)o.x, (double)o.y, (double)o.z, 1.0},
                                          rt_vec4d{(double)d.x, (double)d.y, (double)d.z, 0.0}};
                else // (a miss by rt_render_rays' rule: a zero direction)
                    rays_out[at] = rt_ray{rt_vec4d{0.0, 0.0, 0.0, 0.0}, rt_vec4d{0.0, 0.0, 0.0, 0.0}};
            }
        }
    });
    return RT_OK;
}

int rt_camera_beams(const rt_camera* cam, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w, int32_t h,
                    rt_beam* out)
{
    if (!cam || !out || (cam->kind != RT_CAMERA_FRUSTUM && cam->kind != RT_CAMERA_ORTHO) || width <= 0 || height <= 0 ||
        w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || (int64_t)x0 + w > width || (int64_t)y0 + h > height) {
        set_error("rt_camera_beams: bad argument (null pointer, unknown camera kind, w or h <= 0, or a tile outside the frame)");
        return RT_ERR_ARG;
    }
    CameraD c;
    CameraF camf;
    camera_init(*cam, width, height, c, camf);
    const Vec4d zero = v4d(0.0, 0.0, 0.0, 0.0);
    for (int x = 0; x < w; x++)
        for (int y = 0; y < h; y++) {
            const double fx = (double)(x0 + x), fy = (double)(y0 + y);
            rt_beam& B = out[(size_t)x * h + y];
            if (c.kind == RT_CAMERA_FRUSTUM) { // camera_ray_d's vector before its normalisation, and its steps per pixel
                const double ox = c.tan_x * ((fx - c.w2) / c.w2), oy = c.tan_y * ((fy - c.h2) / c.h2);
                B.origin = vec4(c.position, 1.0);
                B.direction = vec4(add(add(c.look, scale(c.side, ox)), scale(c.up, oy)), 0.0);
                B.origin_du = B.origin_dv = vec4(zero, 0.0);
                B.direction_du = vec4(scale(c.side, c.tan_x / c.w2), 0.0);
                B.direction_dv = vec4(scale(c.up, c.tan_y / c.h2), 0.0);
            } else {
                B.origin = vec4(add(add(c.position, scale(c.side, (fx - c.w2) * c.h_mult)), scale(c.up, (fy - c.h2) * c.v_mult)), 1.0);
                B.direction = vec4(c.look, 0.0);
                B.origin_du = vec4(scale(c.side, c.h_mult), 0.0);
                B.origin_dv = vec4(scale(c.up, c.v_mult), 0.0);
                B.direction_du = B.direction_dv = vec4(zero, 0.0);
            }
        }
    return RT_OK;
}

} // extern "C"
