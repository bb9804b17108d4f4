// api_denoise.hip -- the C ABI's denoising pass (include/rtcore.h, "denoising"): an edge-avoiding a-trous
// filter over whole-frame accumulators with moments, guided by first hits and the pixels' own variance
// estimate, and its host twin, the same definition compiled for the CPU.
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "rt_scene.h"

namespace {

#define DN_HD __host__ __device__ inline

// What a level reads of a pixel: 32 B of guides (prim < 0: the pixel is invalid, whatever its hit says)
// and 16 B of state.  Both are moved as whole 16-byte rows.
struct alignas(16) DnGuide {
    float nx, ny, nz, d;
    float px, py, pz;
    int32_t prim;
};
struct alignas(16) DnState {
    float r, g, b, v;
};
static_assert(sizeof(DnGuide) == 32 && sizeof(DnState) == 16, "denoise records");

// IEEE division and square root on both sides.  On the device `/` and __builtin_sqrtf are the correctly
// rounded expansions (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt; the Makefile passes no
// fast-math flag).  __fsqrt_rn is not used: this toolchain's header maps it to the native approximation.
DN_HD float dn_div(float a, float b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
DN_HD float dn_sqrt(float a)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_sqrtf(a);
#else
    return std::sqrt(a);
#endif
}
DN_HD bool dn_finite(float x) { return x >= -3.4028234663852886e38f && x <= 3.4028234663852886e38f; } // (NaN: false)
DN_HD float dn_abs(float x) { return x < 0.0f ? -x : x; }
DN_HD float dn_lum(const DnState& s)
{
#pragma clang fp contract(off)
    return 0.299f * s.r + 0.587f * s.g + 0.114f * s.b;
}
// f(t) = 1 / (1 + t + 0.5 t t) for t >= 0, else 0 (NaN: 0)
DN_HD float dn_f(float t)
{
#pragma clang fp contract(off)
    return t >= 0.0f ? dn_div(1.0f, 1.0f + t + 0.5f * t * t) : 0.0f;
}
// w_n of rtcore.h
DN_HD float dn_wn(const rt_denoise_params& P, const DnGuide& p, const DnGuide& q)
{
#pragma clang fp contract(off)
    if ((P.flags & RT_DENOISE_SAME_PRIM) && q.prim != p.prim) return 0.0f;
    const float dot = p.nx * q.nx + p.ny * q.ny + p.nz * q.nz;
    float m = dot > 0.0f ? dot : 0.0f;
    for (int k = 0; k < P.normal_pow_log2; k++) m = m * m;
    return m;
}

// The preparation of rtcore.h for one pixel, from its accumulators and its first hit.
DN_HD void denoise_prepare(double sr, double sg, double sb, uint32_t ns, uint32_t nm, double Q, uint32_t J, const rt_hit& hit,
                           DnGuide& G, DnState& S)
{
#pragma clang fp contract(off)
    S = DnState{0.0f, 0.0f, 0.0f, 0.0f};
    bool valid = ns > 0 && hit.prim_id >= 0;
    if (valid) {
        const double n = (double)ns;
        const double N = (double)((uint64_t)ns + (uint64_t)nm);
        const double Y = 0.299 * sr + 0.587 * sg + 0.114 * sb;
        double v;
        if (J >= 2) {
            const double d = (Q - Y * Y / N) / (double)(J - 1);
            const double s2 = d > 0.0 ? d : 0.0;
            v = s2 * N / (n * n);
        } else {
            const double m = Y / n;
            v = m * m;
        }
        const DnState c{(float)(sr / n), (float)(sg / n), (float)(sb / n), (float)v};
        valid = dn_finite(c.r) && dn_finite(c.g) && dn_finite(c.b) && dn_finite(c.v);
        if (valid) S = c;
    }
    G = DnGuide{hit.normal[0], hit.normal[1], hit.normal[2], (float)hit.distance,
                hit.position[0], hit.position[1], hit.position[2], valid ? hit.prim_id : -1};
}

// One level of rtcore.h for the valid pixel (x, y) with guides Gp and state Sp; F(qx, qy, G) gives a frame
// pixel's guides and F(qx, qy, S) its state.
template <class Fetch>
DN_HD DnState denoise_level(const rt_denoise_params& P, int x, int y, int w, int h, int s, const Fetch& F, const DnGuide& Gp,
                            const DnState& Sp)
{
#pragma clang fp contract(off)
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    const float h5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float gs = 0.0f, ks = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; j++)
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const float kw = k3[i + 1] * k3[j + 1];
            float v = Sp.v;
            if (i != 0 || j != 0) {
                const int qx = x + i, qy = y + j;
                if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                DnGuide Gq;
                F(qx, qy, Gq);
                if (Gq.prim < 0 || !(dn_wn(P, Gp, Gq) > 0.0f)) continue;
                DnState Sq;
                F(qx, qy, Sq);
                v = Sq.v;
            }
            gs += kw * v;
            ks += kw;
        }
    const float den_l = P.sigma_l * dn_sqrt(dn_div(gs, ks)) + P.lum_eps;
    const float den_z = P.sigma_z * Gp.d;
    const float Lp = dn_lum(Sp);
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; j++)
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            if (i == 0 && j == 0) {
                const float wc = 0.140625f; // h(0) h(0) = 9/64
                sw += wc;
                sv += wc * wc * Sp.v;
                continue;
            }
            const int qx = x + s * i, qy = y + s * j;
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
            DnGuide Gq;
            F(qx, qy, Gq);
            if (Gq.prim < 0) continue;
            const float wn = dn_wn(P, Gp, Gq);
            if (!(wn > 0.0f)) continue; // (the product below would be 0 or NaN)
            const float dx = Gq.px - Gp.px, dy = Gq.py - Gp.py, dz = Gq.pz - Gp.pz;
            const float wz = dn_f(dn_div(dn_abs(Gp.nx * dx + Gp.ny * dy + Gp.nz * dz), den_z));
            DnState Sq;
            F(qx, qy, Sq);
            const float wl = dn_f(dn_div(dn_abs(dn_lum(Sq) - Lp), den_l));
            const float wt = h5[i + 2] * h5[j + 2] * wn * wz * wl;
            if (!(wt > 0.0f)) continue;
            sw += wt;
            sr += wt * (Sq.r - Sp.r);
            sg += wt * (Sq.g - Sp.g);
            sb += wt * (Sq.b - Sp.b);
            sv += wt * wt * Sq.v;
        }
    return DnState{Sp.r + dn_div(sr, sw), Sp.g + dn_div(sg, sw), Sp.b + dn_div(sb, sw), dn_div(sv, sw * sw)};
}

// The accumulators a call reads and the outputs it writes, in rt_render_pixels_device's layout.
struct DnFrame {
    const double* sum;
    const uint32_t* samples;
    const uint32_t* misses;
    const double* q;
    const uint32_t* batches;
    const rt_hit* hits;
    double* out_sum;
    float* out_var;
    size_t plane, npix;
    int w, h;
};

// The output of rtcore.h for pixel a after the last level (S: its state then; G.prim < 0: pass through).
DN_HD void denoise_output(const DnFrame& A, size_t a, const DnGuide& G, const DnState& S)
{
#pragma clang fp contract(off)
    if (G.prim >= 0) {
        const double n = (double)A.samples[a];
        A.out_sum[a] = (double)S.r * n;
        A.out_sum[A.plane + a] = (double)S.g * n;
        A.out_sum[2 * A.plane + a] = (double)S.b * n;
    } else {
        A.out_sum[a] = A.sum[a];
        A.out_sum[A.plane + a] = A.sum[A.plane + a];
        A.out_sum[2 * A.plane + a] = A.sum[2 * A.plane + a];
    }
    if (A.out_var) A.out_var[a] = G.prim >= 0 ? S.v : 0.0f;
}

// A frame pixel's records from the arrays of the whole frame (the host twin, and the device's levels
// whose halo is wider than a tile).
struct FrameFetch {
    const DnGuide* guides;
    const DnState* state;
    int w;
    DN_HD void operator()(int qx, int qy, DnGuide& G) const
    {
        const size_t a = (size_t)qy * (size_t)w + (size_t)qx;
#ifdef __HIP_DEVICE_COMPILE__
        const float4* g = reinterpret_cast<const float4*>(guides) + 2 * a;
        const float4 r0 = g[0], r1 = g[1];
        G = DnGuide{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, __float_as_int(r1.w)};
#else
        G = guides[a];
#endif
    }
    DN_HD void operator()(int qx, int qy, DnState& S) const
    {
        const size_t a = (size_t)qy * (size_t)w + (size_t)qx;
#ifdef __HIP_DEVICE_COMPILE__
        const float4 r = reinterpret_cast<const float4*>(state)[a];
        S = DnState{r.x, r.y, r.z, r.w};
#else
        S = state[a];
#endif
    }
};

// ---- the device pass ----

// Preparation: 92 B read per pixel, one guide record and one state record written.
__global__ void __launch_bounds__(256) denoise_prepare_kernel(DnFrame A, DnGuide* __restrict__ guides, DnState* __restrict__ state)
{
    const size_t a = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (a >= A.npix) return;
    const float4* hp = reinterpret_cast<const float4*>(A.hits) + 3 * a; // rt_hit: three 16-byte rows
    const float4 h0 = hp[0], h1 = hp[1], h2 = hp[2];
    rt_hit hit;
    hit.prim_id = __float_as_int(h0.x);
    hit.inside = __float_as_int(h0.y);
    hit.distance = __hiloint2double(__float_as_int(h0.w), __float_as_int(h0.z));
    hit.position[0] = h1.x, hit.position[1] = h1.y, hit.position[2] = h1.z;
    hit.normal[0] = h1.w, hit.normal[1] = h2.x, hit.normal[2] = h2.y;
    DnGuide G;
    DnState S;
    denoise_prepare(A.sum[a], A.sum[A.plane + a], A.sum[2 * A.plane + a], A.samples[a], A.misses[a], A.q[a], A.batches[a], hit,
                    G, S);
    float4* gp = reinterpret_cast<float4*>(guides) + 2 * a;
    gp[0] = make_float4(G.nx, G.ny, G.nz, G.d);
    gp[1] = make_float4(G.px, G.py, G.pz, __int_as_float(G.prim));
    reinterpret_cast<float4*>(state)[a] = make_float4(S.r, S.g, S.b, S.v);
}

// A workgroup's tile is kTileW x kTileH pixels at a multiple of (kTileW, kTileH), so every row of it is
// kTileW * 16 B of consecutive state records and twice that of guides; a thread computes the pixels
// (t & 31, (t >> 5) + 8 r), r = 0, 1.
constexpr int kTileW = 32, kTileH = 16;

struct LevelArgs {
    rt_denoise_params P;
    DnFrame F;
    const DnGuide* guides;
    const DnState* in;
    DnState* out;   // null on the last level: the outputs are written instead
    int step, tiles_x;
};

// A tile's records, halo included, staged in LDS as three planes of 16-byte rows (a wave reads
// consecutive rows of one plane: ds_read_b128 without bank conflicts).
template <int S>
struct TileFetch {
    static constexpr int kW = kTileW + 4 * S, kH = kTileH + 4 * S;
    const float4* g0;
    const float4* g1;
    const float4* st;
    int ox, oy;
    __device__ void operator()(int qx, int qy, DnGuide& G) const
    {
        const int a = (qy - oy) * kW + (qx - ox);
        const float4 r0 = g0[a], r1 = g1[a];
        G = DnGuide{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, __float_as_int(r1.w)};
    }
    __device__ void operator()(int qx, int qy, DnState& s) const
    {
        const float4 r = st[(qy - oy) * kW + (qx - ox)];
        s = DnState{r.x, r.y, r.z, r.w};
    }
};

template <class Fetch>
__device__ inline void level_pixel(const LevelArgs& A, const Fetch& F, int x, int y)
{
    if (x >= A.F.w || y >= A.F.h) return;
    const size_t a = (size_t)y * (size_t)A.F.w + (size_t)x;
    DnGuide G;
    DnState S;
    F(x, y, G);
    F(x, y, S);
    if (G.prim >= 0) S = denoise_level(A.P, x, y, A.F.w, A.F.h, A.step, F, G, S);
    if (A.out) reinterpret_cast<float4*>(A.out)[a] = make_float4(S.r, S.g, S.b, S.v);
    else denoise_output(A.F, a, G, S);
}

// Level with step S in {1, 2, 4}: the tile and its 2 S halo are staged in LDS, (kTileW + 4 S) x
// (kTileH + 4 S) records of 48 B (34.6, 46.1 and 73.7 KB), so a record is read from memory 1.4 to 3 times
// per level and not 25.  S = 0: any step, every tap read from memory (L2 and the last-level cache hold
// the frame); for steps from 8 up the halo would be larger than the tile.
template <int S>
__global__ void __launch_bounds__(256) denoise_level_kernel(LevelArgs A)
{
    const int t = threadIdx.x;
    const int by = (int)(blockIdx.x / (unsigned)A.tiles_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)A.tiles_x);
    const int x = bx * kTileW + (t & 31), y = by * kTileH + (t >> 5);
    if constexpr (S == 0) {
        const FrameFetch F{A.guides, A.in, A.F.w};
        level_pixel(A, F, x, y);
        level_pixel(A, F, x, y + 8);
    } else {
        using T = TileFetch<S>;
        __shared__ float4 tile[3 * T::kW * T::kH];
        const int ox = bx * kTileW - 2 * S, oy = by * kTileH - 2 * S;
        const float4* g4 = reinterpret_cast<const float4*>(A.guides);
        const float4* s4 = reinterpret_cast<const float4*>(A.in);
        // a tile without a valid pixel (background) only passes through: no halo is staged for it
        int valid = 0;
        if (x < A.F.w) {
            if (y < A.F.h) valid |= A.guides[(size_t)y * (size_t)A.F.w + (size_t)x].prim >= 0;
            if (y + 8 < A.F.h) valid |= A.guides[(size_t)(y + 8) * (size_t)A.F.w + (size_t)x].prim >= 0;
        }
        if (!__syncthreads_or(valid)) {
            const FrameFetch F{A.guides, A.in, A.F.w};
            level_pixel(A, F, x, y);
            level_pixel(A, F, x, y + 8);
            return;
        }
        for (int i = t; i < T::kW * T::kH; i += 256) {
            const int ly = i / T::kW, lx = i - ly * T::kW;
            const int gx = ox + lx, gy = oy + ly;
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), rs = r0;
            if (gx >= 0 && gy >= 0 && gx < A.F.w && gy < A.F.h) {
                const size_t a = (size_t)gy * (size_t)A.F.w + (size_t)gx;
                r0 = g4[2 * a];
                r1 = g4[2 * a + 1];
                rs = s4[a];
            }
            tile[i] = r0;
            tile[T::kW * T::kH + i] = r1;
            tile[2 * T::kW * T::kH + i] = rs;
        }
        __syncthreads();
        const T F{tile, tile + T::kW * T::kH, tile + 2 * T::kW * T::kH, ox, oy};
        level_pixel(A, F, x, y);
        level_pixel(A, F, x, y + 8);
    }
}

// The pass's temporary memory, the library's own, one per device: the guides and two state buffers.
// Calls on one device share it, so a call on another stream than the last is ordered after it.
struct DenoiseScratch {
    DnGuide* guides = nullptr;
    DnState* state[2] = {nullptr, nullptr};
    size_t npix = 0;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool any = false;
};
constexpr int kMaxDevices = 64;
DenoiseScratch g_scratch[kMaxDevices]; // (never freed: the runtime may be gone when statics are destroyed)
std::mutex g_scratch_mutex;

int check_denoise(const char* name, const rt_denoise_params* P, const double* sum, const void* samples, const void* misses,
                  const void* q, const void* batches, uint64_t plane, const void* hits, int32_t w, int32_t h,
                  const double* out_sum)
{
    const char* bad = nullptr;
    if (!P || !sum || !samples || !misses || !q || !batches || !hits || !out_sum) bad = "null pointer";
    else if (w <= 0 || h <= 0) bad = "a frame of no pixels";
    else if ((uint64_t)w * (uint64_t)h >= (1ull << 32)) bad = "a frame of 2^32 pixels or more";
    else if (plane != 0 && plane < (uint64_t)w * (uint64_t)h) bad = "plane smaller than the frame";
    else if (!(P->sigma_l > 0.0f) || !(P->sigma_z > 0.0f) || !(P->lum_eps > 0.0f)) bad = "sigma_l, sigma_z or lum_eps not above 0";
    else if (P->normal_pow_log2 < 0 || P->normal_pow_log2 > 8) bad = "normal_pow_log2 outside 0 .. 8";
    else if (P->iterations < 1 || P->iterations > 5) bad = "iterations outside 1 .. 5";
    else if (P->flags & ~RT_DENOISE_SAME_PRIM) bad = "unknown flag bits";
    else if (P->reserved[0] || P->reserved[1]) bad = "reserved not 0";
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

void launch_level(const LevelArgs& A, hipStream_t st)
{
    const dim3 grid((unsigned)A.tiles_x * (unsigned)((A.F.h + kTileH - 1) / kTileH)), block(256);
    // steps 1 and 2 stage their tile in LDS; step 4 measured 0.015 ms slower staged (its 73.7 KB leave two
    // workgroups per CU) than read from memory.  RTCORE_DENOISE_LDS = the largest step that is
    // staged (0: none, 4: step 4 too), for A/B measurements
    int staged = 2;
    if (const char* e = getenv("RTCORE_DENOISE_LDS")) staged = atoi(e);
    switch (A.step <= staged ? A.step : 0) {
    case 1: hipLaunchKernelGGL(denoise_level_kernel<1>, grid, block, 0, st, A); break;
    case 2: hipLaunchKernelGGL(denoise_level_kernel<2>, grid, block, 0, st, A); break;
    case 4: hipLaunchKernelGGL(denoise_level_kernel<4>, grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL(denoise_level_kernel<0>, grid, block, 0, st, A); break;
    }
}

} // namespace

extern "C" {

int rt_denoise_device(const rt_denoise_params* P, const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses,
                      const double* d_q, const uint32_t* d_batches, uint64_t plane, const rt_hit* d_hits, int32_t width,
                      int32_t height, double* d_out_sum, float* d_out_var, void* stream)
{
    const int rc = check_denoise("rt_denoise_device", P, d_sum, d_samples, d_misses, d_q, d_batches, plane, d_hits, width, height,
                                 d_out_sum);
    if (rc != RT_OK) return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) {
        set_error("rt_denoise_device: device index out of range");
        return RT_ERR_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t npix = (size_t)width * (size_t)height;
    const DnFrame F{d_sum, d_samples, d_misses, d_q, d_batches, d_hits, d_out_sum, d_out_var, plane ? (size_t)plane : npix, npix,
                    width, height};
    std::lock_guard<std::mutex> lock(g_scratch_mutex);
    DenoiseScratch& S = g_scratch[dev];
    if (!S.done) HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    if (npix > S.npix) { // (hipFree waits for the device, so no queued pass still reads the old arrays)
        if (S.guides) (void)hipFree(S.guides);
        for (DnState*& p : S.state)
            if (p) (void)hipFree(p);
        S.guides = nullptr;
        S.state[0] = S.state[1] = nullptr;
        S.npix = 0;
        HIP_TRY(hipMalloc(&S.guides, npix * sizeof(DnGuide)));
        HIP_TRY(hipMalloc(&S.state[0], npix * sizeof(DnState)));
        HIP_TRY(hipMalloc(&S.state[1], npix * sizeof(DnState)));
        S.npix = npix;
    }
    if (S.any && st != S.last) HIP_TRY(hipStreamWaitEvent(st, S.done, 0));
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, F, S.guides, S.state[0]);
    for (int k = 0; k < P->iterations; k++) {
        const LevelArgs A{*P, F, S.guides, S.state[k & 1], k + 1 < P->iterations ? S.state[(k + 1) & 1] : nullptr, 1 << k,
                          (width + kTileW - 1) / kTileW};
        launch_level(A, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.done, st));
    S.last = st;
    S.any = true;
    return RT_OK;
}

int rt_debug_denoise(const rt_denoise_params* P, const double* sum, const uint32_t* samples, const uint32_t* misses,
                     const double* q, const uint32_t* batches, uint64_t plane, const rt_hit* hits, int32_t width, int32_t height,
                     double* out_sum, float* out_var)
{
    const int rc = check_denoise("rt_debug_denoise", P, sum, samples, misses, q, batches, plane, hits, width, height, out_sum);
    if (rc != RT_OK) return rc;
    const size_t npix = (size_t)width * (size_t)height, pl = plane ? (size_t)plane : npix;
    const DnFrame F{sum, samples, misses, q, batches, hits, out_sum, out_var, pl, npix, width, height};
    std::vector<DnGuide> guides(npix);
    std::vector<DnState> state[2] = {std::vector<DnState>(npix), std::vector<DnState>(P->iterations > 1 ? npix : 0)};
    for (size_t a = 0; a < npix; a++)
        denoise_prepare(sum[a], sum[pl + a], sum[2 * pl + a], samples[a], misses[a], q[a], batches[a], hits[a], guides[a],
                        state[0][a]);
    for (int k = 0; k < P->iterations; k++) {
        const FrameFetch fetch{guides.data(), state[k & 1].data(), width};
        const bool last = k + 1 == P->iterations;
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t a = (size_t)y * (size_t)width + (size_t)x;
                DnState S = state[k & 1][a];
                if (guides[a].prim >= 0) S = denoise_level(*P, x, y, width, height, 1 << k, fetch, guides[a], S);
                if (last) denoise_output(F, a, guides[a], S);
                else state[(k + 1) & 1][a] = S;
            }
    }
    return RT_OK;
}

} // extern "C"
