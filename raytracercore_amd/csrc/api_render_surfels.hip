// api_render_surfels.hip -- the C ABI's radiance queries for surfels (include/rtcore.h, "radiance
// queries", rt_surfel): rt_render_rays with the sample's direction drawn on the device about the
// surfel's normal, by the SURFELS instances of the path kernels (kernels_path.hip, refill).  The entry
// points' bodies are rt_render_rays' (api_render_rays.hip): a surfel has an rt_ray's size, so the list
// buffers, the chunks and the staging are the rays' own.  Here too: the kernel that reports the sample
// rays (rt_debug_surfel_rays_device), a second compilation of the path kernels' function (rt_surfel.h).
#include "rt_scene.h"
#include "rt_surfel.h"

static_assert(sizeof(rt_surfel) == sizeof(rt_ray) && sizeof(rt_surfel) == 64, "rt_surfel: four 16-byte rows, an rt_ray's size");

namespace {

constexpr int64_t kSurfelsChunk = 1 << 19; // surfels of one chunk of rt_render_surfels (rt_render_rays' size and variable)

bool known_mode(int32_t mode) { return mode == RT_GATHER_DIFFUSE || mode == RT_GATHER_COSINE || mode == RT_GATHER_SPHERE; }

int bad_mode(const char* name)
{
    set_error(std::string(name) + ": bad argument (unknown gather mode)");
    return RT_ERR_ARG;
}

// The sample start of the SURFELS instances (refill), one thread per sample: the same draws and the
// same function of rt_surfel.h on the same inputs; the ray widened, or zeros for an invalid surfel.
__global__ void __launch_bounds__(256) surfel_rays_kernel(const double2* __restrict__ surfels, unsigned long long total, unsigned spp,
                                                          int mode, rt_key2 seed_key, unsigned long long sample_base,
                                                          unsigned long long stream_base, double2* __restrict__ out)
{
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long at = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; at < total; at += step) {
        const unsigned long long i = at / spp, k = at - i * spp;
        rt_rng rng = rt_rng_from_pixel_key(rt_rng_pixel_key(seed_key, stream_base + i), sample_base + k);
        const float u1 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        const float u2 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        V3 o, d;
        double2* const row = out + 4 * at;
        if (surfel_sample(surfels + 4 * i, mode, u1, u2, o, d)) {
            row[0] = make_double2((double)o.x, (double)o.y);
            row[1] = make_double2((double)o.z, 1.0);
            row[2] = make_double2((double)d.x, (double)d.y);
            row[3] = make_double2((double)d.z, 0.0);
        } else { // (a miss by rt_render_rays' rule: a zero direction)
            row[0] = row[1] = row[2] = row[3] = make_double2(0.0, 0.0);
        }
    }
}

} // namespace

namespace rtc { // (declared in rt_scene.h: api_probe_depth.hip makes its sample rays by the same launch)

int launch_surfel_rays(int32_t mode, const rt_surfel* d_surfels, unsigned long long total, unsigned spp, uint64_t seed,
                       uint64_t sample_base, uint64_t stream_base, rt_ray* d_rays_out, hipStream_t st)
{
    const unsigned blocks = (unsigned)std::min<unsigned long long>((total + 255) / 256, 1u << 16);
    surfel_rays_kernel<<<blocks, 256, 0, st>>>(reinterpret_cast<const double2*>(d_surfels), total, spp, mode, rt_rng_seed_key(seed),
                                               sample_base, stream_base, reinterpret_cast<double2*>(d_rays_out));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

} // namespace rtc

extern "C" {

int rt_render_surfels_device(rt_scene* s, int32_t mode, const rt_surfel* d_surfels, int64_t n, int32_t spp, uint64_t seed,
                             uint64_t sample_base, uint64_t stream_base, double* d_sum, uint32_t* d_samples,
                             uint32_t* d_misses, unsigned long long* d_count, void* stream)
{
    if (!known_mode(mode)) return bad_mode("rt_render_surfels_device");
    const RenderList kind = {ITEMS_SURFELS, sizeof(rt_surfel), kSurfelsChunk, "surfels", mode};
    return render_list_device(s, kind, "rt_render_surfels_device", d_surfels, n, spp, seed, sample_base, stream_base, d_sum,
                              d_samples, d_misses, d_count, stream);
}

int rt_render_surfels(rt_scene* s, int32_t mode, const rt_surfel* surfels, int64_t n, int32_t spp, uint64_t seed,
                      uint64_t sample_base, uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses,
                      uint64_t* rays_out)
{
    if (!known_mode(mode)) return bad_mode("rt_render_surfels");
    const RenderList kind = {ITEMS_SURFELS, sizeof(rt_surfel), kSurfelsChunk, "surfels", mode};
    return render_list_host(s, kind, "rt_render_surfels", surfels, n, spp, seed, sample_base, stream_base, sum_rgb, samples,
                            misses, rays_out);
}

int rt_debug_surfel_rays_device(int32_t mode, const rt_surfel* d_surfels, int64_t n, int32_t spp, uint64_t seed,
                                uint64_t sample_base, uint64_t stream_base, rt_ray* d_rays_out, void* stream)
{
    if (!known_mode(mode)) return bad_mode("rt_debug_surfel_rays_device");
    if (n < 0 || spp <= 0 || (n > 0 && (!d_surfels || !d_rays_out))) {
        set_error("rt_debug_surfel_rays_device: bad argument (null pointer, n < 0 or spp <= 0)");
        return RT_ERR_ARG;
    }
    if (n == 0) return RT_OK;
    if ((unsigned long long)n > (1ull << 57) / (unsigned long long)spp) { // (the byte offsets of 64 B per sample stay in 64 bits)
        set_error("rt_debug_surfel_rays_device: n x spp too large");
        return RT_ERR_ARG;
    }
    return launch_surfel_rays(mode, d_surfels, (unsigned long long)n * (unsigned long long)spp, (unsigned)spp, seed, sample_base,
                              stream_base, d_rays_out, static_cast<hipStream_t>(stream));
}

} // extern "C"
