// api_reproject.hip -- the C ABI's temporal reprojection (include/rtcore.h, "temporal reprojection"): a
// nearest-pixel gather that carries whole-frame accumulators with moments from the pixels of a previous
// camera to the pixels of the current one, validated against both cameras' first hits, and its host twin,
// the same definition compiled for the CPU.
#include <cstdint>

#include "rt_scene.h"

namespace {

#define RP_HD __host__ __device__ inline

RP_HD bool rp_finite(float x) { return x >= -3.4028234663852886e38f && x <= 3.4028234663852886e38f; } // (NaN: false)
RP_HD float rp_abs(float x) { return x < 0.0f ? -x : x; }
RP_HD double rp_lum(double r, double g, double b)
{
#pragma clang fp contract(off)
    return 0.299 * r + 0.587 * g + 0.114 * b;
}

// Steps 1 and 2 of rtcore.h: the previous camera's pixel (qx, qy) that shows the current hit H, or false.
RP_HD bool reproject_project(const CameraD& C, const rt_hit& H, int w, int h, int& qx, int& qy)
{
#pragma clang fp contract(off)
    if (H.prim_id < 0 || !rp_finite(H.position[0]) || !rp_finite(H.position[1]) || !rp_finite(H.position[2])) return false;
    const double vx = (double)H.position[0] - C.position.x, vy = (double)H.position[1] - C.position.y,
                 vz = (double)H.position[2] - C.position.z;
    const double z = vx * C.look.x + vy * C.look.y + vz * C.look.z;
    const double a = vx * C.side.x + vy * C.side.y + vz * C.side.z;
    const double b = vx * C.up.x + vy * C.up.y + vz * C.up.z;
    if (!(z > 0.0)) return false;
    double fx, fy;
    if (C.kind == RT_CAMERA_FRUSTUM) {
        fx = C.w2 + C.w2 * ((a / z) / C.tan_x);
        fy = C.h2 + C.h2 * ((b / z) / C.tan_y);
    } else {
        fx = C.w2 + a / C.h_mult;
        fy = C.h2 + b / C.v_mult;
    }
    if (!(fx >= -0.5 && fx < (double)w - 0.5 && fy >= -0.5 && fy < (double)h - 0.5)) return false;
    qx = (int)(fx + 0.5);
    qy = (int)(fy + 0.5);
    // (a frame one pixel wide or high: fx + 0.5 may round up to 1.0)
    if (qx >= w) qx = w - 1;
    if (qy >= h) qy = h - 1;
    return true;
}

// Step 3 of rtcore.h: may the current hit H take the history of the previous camera's hit G?
RP_HD bool reproject_accept(const rt_reproject_params& P, const rt_hit& H, const rt_hit& G)
{
#pragma clang fp contract(off)
    if (G.prim_id < 0) return false;
    if ((P.flags & RT_REPROJECT_SAME_PRIM) && G.prim_id != H.prim_id) return false;
    if (G.inside != H.inside) return false;
    const float dot = H.normal[0] * G.normal[0] + H.normal[1] * G.normal[1] + H.normal[2] * G.normal[2];
    if (!(dot >= P.normal_cos_min)) return false;
    const float dx = G.position[0] - H.position[0], dy = G.position[1] - H.position[1], dz = G.position[2] - H.position[2];
    const float pd = rp_abs(H.normal[0] * dx + H.normal[1] * dy + H.normal[2] * dz);
    return pd <= P.sigma_z * (float)H.distance;
}

// A pixel's five accumulators.
struct RpAcc {
    double r, g, b, q;
    uint32_t ns, nm, nb;
};

// Steps 4 and 5 of rtcore.h on the source pixel's accumulators, in place; false: no history (N == 0).
RP_HD bool reproject_history(const rt_reproject_params& P, RpAcc& A)
{
#pragma clang fp contract(off)
    const uint64_t N = (uint64_t)A.ns + (uint64_t)A.nm;
    if (N == 0) return false;
    if (N <= (uint64_t)P.max_history) return true;
    const uint32_t N1 = P.max_history;
    const uint32_t ns1 = (uint32_t)((uint64_t)A.ns * (uint64_t)N1 / N);
    const double Y = rp_lum(A.r, A.g, A.b);
    if (A.ns > 0) {
        const double f = (double)ns1 / (double)A.ns;
        A.r = A.r * f;
        A.g = A.g * f;
        A.b = A.b * f;
    }
    const double Y1 = rp_lum(A.r, A.g, A.b);
    const double n = (double)N, n1 = (double)N1;
    if (A.nb >= 2) {
        const uint32_t J1 = A.nb < N1 ? A.nb : N1;
        const double D = A.q - Y * Y / n;
        A.q = D * ((double)(J1 - 1) / (double)(A.nb - 1)) + Y1 * Y1 / n1;
        A.nb = J1;
    } else {
        A.q = A.q * (n1 / n);
    }
    A.ns = ns1;
    A.nm = N1 - ns1;
    return true;
}

// What a call reads and writes, in rt_render_pixels_device's layout.
struct RpFrame {
    const rt_hit* prev_hits;
    const rt_hit* hits;
    const double* sum;
    const uint32_t* samples;
    const uint32_t* misses;
    const double* q;
    const uint32_t* batches;
    double* out_sum;
    uint32_t* out_samples;
    uint32_t* out_misses;
    double* out_q;
    uint32_t* out_batches;
    int32_t* out_src;
    size_t plane;
    int w, h, blocks_x, n_blocks;
};

RP_HD RpAcc rp_load(const RpFrame& F, size_t s)
{
    return RpAcc{F.sum[s], F.sum[F.plane + s], F.sum[2 * F.plane + s], F.q[s], F.samples[s], F.misses[s], F.batches[s]};
}

RP_HD void rp_store(const RpFrame& F, size_t a, const RpAcc& A, int32_t src)
{
    F.out_sum[a] = A.r;
    F.out_sum[F.plane + a] = A.g;
    F.out_sum[2 * F.plane + a] = A.b;
    F.out_samples[a] = A.ns;
    F.out_misses[a] = A.nm;
    F.out_q[a] = A.q;
    F.out_batches[a] = A.nb;
    if (F.out_src) F.out_src[a] = src;
}

// The whole definition for the current pixel (x, y); L(hits, a) gives a frame's hit record.
template <class Load>
RP_HD void reproject_pixel(const rt_reproject_params& P, const CameraD& C, const RpFrame& F, int x, int y, const Load& L)
{
    const size_t a = (size_t)y * (size_t)F.w + (size_t)x;
    const rt_hit H = L(F.hits, a);
    RpAcc A{0.0, 0.0, 0.0, 0.0, 0u, 0u, 0u};
    int32_t src = -1;
    int qx, qy;
    if (reproject_project(C, H, F.w, F.h, qx, qy)) {
        const size_t s = (size_t)qy * (size_t)F.w + (size_t)qx;
        if (reproject_accept(P, H, L(F.prev_hits, s))) {
            RpAcc B = rp_load(F, s);
            if (reproject_history(P, B)) {
                A = B;
                src = (int32_t)s;
            }
        }
    }
    rp_store(F, a, A, src);
}

struct HostLoad {
    RP_HD rt_hit operator()(const rt_hit* hits, size_t a) const { return hits[a]; }
};

// ---- the device pass ----

// rt_hit as three 16-byte rows
struct RowLoad {
    __device__ rt_hit operator()(const rt_hit* hits, size_t a) const
    {
        const float4* hp = reinterpret_cast<const float4*>(hits) + 3 * a;
        const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
        rt_hit hit;
        hit.prim_id = __float_as_int(h0.x);
        hit.inside = __float_as_int(h0.y);
        hit.distance = __hiloint2double(__float_as_int(h0.w), __float_as_int(h0.z));
        hit.position[0] = h1.x, hit.position[1] = h1.y, hit.position[2] = h1.z;
        hit.normal[0] = h1.w, hit.normal[1] = h2.x, hit.normal[2] = h2.y;
        hit.reserved[0] = hit.reserved[1] = 0;
        return hit;
    }
};

// One wave per 8x8 block of the frame (four per workgroup, consecutive blocks of a row of blocks): lane l
// is the block's pixel (l & 7, l >> 3), so a wave's gathers land in a compact patch of the previous frame
// and its stores are eight runs of eight consecutive pixels.  The parameters and the camera are kernel
// arguments (SGPRs): the projection's constants are wave-uniform.  No LDS, no atomics; about 140 B read and
// 48 B written per pixel.
__global__ void __launch_bounds__(256) reproject_kernel(rt_reproject_params P, CameraD C, RpFrame F)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= F.n_blocks) return; // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int by = b / F.blocks_x, bx = b - by * F.blocks_x;
    const int x = bx * 8 + (lane & 7), y = by * 8 + (lane >> 3);
    if (x >= F.w || y >= F.h) return;
    reproject_pixel(P, C, F, x, y, RowLoad{});
}

int check_reproject(const char* name, const rt_reproject_params* P, const rt_camera* cam, const void* prev_hits, const void* hits,
                    const double* sum, const void* samples, const void* misses, const void* q, const void* batches, uint64_t plane,
                    int32_t w, int32_t h, const double* out_sum, const void* out_samples, const void* out_misses, const void* out_q,
                    const void* out_batches)
{
    const char* bad = nullptr;
    if (!P || !cam || !prev_hits || !hits || !sum || !samples || !misses || !q || !batches || !out_sum || !out_samples ||
        !out_misses || !out_q || !out_batches)
        bad = "null pointer";
    else if (w <= 0 || h <= 0) bad = "a frame of no pixels";
    else if ((uint64_t)w * (uint64_t)h >= (1ull << 32)) bad = "a frame of 2^32 pixels or more";
    else if (plane != 0 && plane < (uint64_t)w * (uint64_t)h) bad = "plane smaller than the frame";
    else if (cam->kind != RT_CAMERA_FRUSTUM && cam->kind != RT_CAMERA_ORTHO) bad = "unknown camera kind";
    else if (!(P->sigma_z > 0.0f)) bad = "sigma_z not above 0";
    else if (!(P->normal_cos_min >= -1.0f && P->normal_cos_min <= 1.0f)) bad = "normal_cos_min outside -1 .. 1";
    else if (P->max_history == 0) bad = "max_history 0";
    else if (P->flags & ~RT_REPROJECT_SAME_PRIM) bad = "unknown flag bits";
    else if (P->reserved[0] || P->reserved[1] || P->reserved[2] || P->reserved[3]) bad = "reserved not 0";
    else {
        const size_t npix = (size_t)w * (size_t)h, extent = 2 * (plane ? (size_t)plane : npix) + npix;
        if (sum < out_sum + extent && out_sum < sum + extent) bad = "out_sum overlaps sum";
    }
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

RpFrame make_frame(const rt_hit* prev_hits, const rt_hit* hits, const double* sum, const uint32_t* samples, const uint32_t* misses,
                   const double* q, const uint32_t* batches, uint64_t plane, int32_t w, int32_t h, double* out_sum,
                   uint32_t* out_samples, uint32_t* out_misses, double* out_q, uint32_t* out_batches, int32_t* out_src)
{
    RpFrame F{prev_hits, hits, sum, samples, misses, q, batches, out_sum, out_samples, out_misses, out_q, out_batches, out_src,
              plane ? (size_t)plane : (size_t)w * (size_t)h, w, h, (w + 7) / 8, 0};
    F.n_blocks = F.blocks_x * ((h + 7) / 8);
    return F;
}

} // namespace

extern "C" {

int rt_reproject_device(const rt_reproject_params* P, const rt_camera* prev_camera, const rt_hit* d_prev_hits, const rt_hit* d_hits,
                        const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses, const double* d_q,
                        const uint32_t* d_batches, uint64_t plane, int32_t width, int32_t height, double* d_out_sum,
                        uint32_t* d_out_samples, uint32_t* d_out_misses, double* d_out_q, uint32_t* d_out_batches, int32_t* d_out_src,
                        void* stream)
{
    const int rc = check_reproject("rt_reproject_device", P, prev_camera, d_prev_hits, d_hits, d_sum, d_samples, d_misses, d_q,
                                   d_batches, plane, width, height, d_out_sum, d_out_samples, d_out_misses, d_out_q, d_out_batches);
    if (rc != RT_OK) return rc;
    CameraD camd;
    CameraF camf;
    camera_init(*prev_camera, width, height, camd, camf);
    const RpFrame F = make_frame(d_prev_hits, d_hits, d_sum, d_samples, d_misses, d_q, d_batches, plane, width, height, d_out_sum,
                                 d_out_samples, d_out_misses, d_out_q, d_out_batches, d_out_src);
    hipLaunchKernelGGL(reproject_kernel, dim3((unsigned)((F.n_blocks + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), *P,
                       camd, F);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_debug_reproject(const rt_reproject_params* P, const rt_camera* prev_camera, const rt_hit* prev_hits, const rt_hit* hits,
                       const double* sum, const uint32_t* samples, const uint32_t* misses, const double* q, const uint32_t* batches,
                       uint64_t plane, int32_t width, int32_t height, double* out_sum, uint32_t* out_samples, uint32_t* out_misses,
                       double* out_q, uint32_t* out_batches, int32_t* out_src)
{
    const int rc = check_reproject("rt_debug_reproject", P, prev_camera, prev_hits, hits, sum, samples, misses, q, batches, plane,
                                   width, height, out_sum, out_samples, out_misses, out_q, out_batches);
    if (rc != RT_OK) return rc;
    CameraD camd;
    CameraF camf;
    camera_init(*prev_camera, width, height, camd, camf);
    const RpFrame F = make_frame(prev_hits, hits, sum, samples, misses, q, batches, plane, width, height, out_sum, out_samples,
                                 out_misses, out_q, out_batches, out_src);
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) reproject_pixel(*P, camd, F, x, y, HostLoad{});
    return RT_OK;
}

} // extern "C"
