// api_adaptive.hip -- the C ABI's selection pass of adaptive sampling (include/rtcore.h, "adaptive
// sampling"): from whole-frame accumulators with moments (rt_render_pixels_device) the compacted list
// of pixels that still need samples, in the path kernels' 8x8 block order, and its host twin, the same
// rule function compiled for the CPU.
#include <cmath>

#include "rt_scene.h"
#include "select_scan.h"

namespace {

// active(N, Y, Q, J) of rtcore.h, from a pixel's accumulators.  One function for the device pass and the
// host twin; every operation is rounded on its own on both sides (no contraction: a fused Y or Q - Y Y / N
// would move pixels at the threshold on one side only), and division and square root are IEEE on both.
// NaN in sum or q: the variance's max(0, .) and the threshold's max(., lum_floor) are written so that a
// NaN operand gives 0 and lum_floor, se = 0 is not above the threshold, and the pixel is inactive.
__host__ __device__ inline bool adaptive_active(const rt_adaptive_params& P, double sr, double sg, double sb, uint32_t ns,
                                                uint32_t nm, double Q, uint32_t J)
{
#pragma clang fp contract(off)
    const uint64_t N = (uint64_t)ns + (uint64_t)nm;
    if (N < P.min_samples) return true;
    if (N >= P.max_samples) return false;
    if (J < 2) return true;
    const double n = (double)N;
    const double Y = 0.299 * sr + 0.587 * sg + 0.114 * sb;
    const double d = (Q - Y * Y / n) / (double)(J - 1);
    const double var = d > 0.0 ? d : 0.0;
    const double mean = Y / n;
    const double level = mean > P.lum_floor ? mean : P.lum_floor;
#ifdef __HIP_DEVICE_COMPILE__
    const double se = __dsqrt_rn(var / n);
#else
    const double se = std::sqrt(var / n);
#endif
    return se > P.rel_tol * level;
}

struct SelectArgs {
    rt_adaptive_params P;
    const double* sum;
    const uint32_t* samples;
    const uint32_t* misses;
    const double* q;
    const uint32_t* batches;
    size_t plane;
    int w, h, blocks_x, n_blocks;
};

// One wave per 8x8 block of the frame (four per workgroup): lane l is the block's pixel
// (x & 7, y & 7) = (l & 7, l >> 3), the path kernels' own order.  The block's active lanes as a ballot
// mask, and their number.
__global__ void __launch_bounds__(256) adaptive_count_kernel(SelectArgs A, unsigned long long* masks, unsigned int* counts)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= A.n_blocks) return; // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int by = b / A.blocks_x, bx = b - by * A.blocks_x;
    const int x = bx * 8 + (lane & 7), y = by * 8 + (lane >> 3);
    bool act = false;
    if (x < A.w && y < A.h) {
        const size_t a = (size_t)y * (size_t)A.w + (size_t)x;
        act = adaptive_active(A.P, A.sum[a], A.sum[A.plane + a], A.sum[2 * A.plane + a], A.samples[a], A.misses[a], A.q[a],
                              A.batches[a]);
    }
    const unsigned long long m = __ballot(act);
    if (lane == 0) {
        masks[b] = m;
        counts[b] = (unsigned)__popcll(m);
    }
}

// Exclusive scan of the n block counts, in place, by one workgroup of 1024: each thread sums a run of
// consecutive counts, the runs' sums are scanned in LDS, and each thread writes its run's offsets.
// *total gets the sum (the number of active pixels).
__global__ void __launch_bounds__(1024) adaptive_scan_kernel(unsigned int* counts, int n, unsigned int* total)
{
    __shared__ unsigned int run[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int i0 = min(n, t * per), i1 = min(n, i0 + per);
    unsigned int s = 0;
    for (int i = i0; i < i1; i++) s += counts[i];
    run[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { // Hillis-Steele, inclusive
        const unsigned int v = t >= d ? run[t - d] : 0u;
        __syncthreads();
        run[t] += v;
        __syncthreads();
    }
    unsigned int off = run[t] - s;
    for (int i = i0; i < i1; i++) {
        const unsigned int c = counts[i];
        counts[i] = off;
        off += c;
    }
    if (t == 1023) *total = run[1023];
}

// The write: block b's active pixels, in lane order, at offs[b] + the lane's rank in the mask; entries
// at or past cap are dropped.
__global__ void __launch_bounds__(256) adaptive_write_kernel(SelectArgs A, const unsigned long long* masks,
                                                             const unsigned int* offs, uint32_t* pixels, uint32_t cap)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= A.n_blocks) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long m = masks[b];
    if (!((m >> lane) & 1ull)) return;
    const unsigned int at = offs[b] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (at >= cap) return;
    const int by = b / A.blocks_x, bx = b - by * A.blocks_x;
    pixels[at] = (uint32_t)(by * 8 + (lane >> 3)) * (uint32_t)A.w + (uint32_t)(bx * 8 + (lane & 7));
}

constexpr int kMaxDevices = 64;
SelectScratch g_scratch[kMaxDevices]; // (never freed: the runtime may be gone when statics are destroyed)
std::mutex g_scratch_mutex;

int check_select(const char* name, const rt_adaptive_params* P, const void* sum, const void* samples, const void* misses,
                 const void* q, const void* batches, int32_t w, int32_t h, const void* pixels, uint32_t cap)
{
    const char* bad = nullptr;
    if (!P || !sum || !samples || !misses || !q || !batches || (!pixels && cap > 0)) bad = "null pointer";
    else if (w <= 0 || h <= 0) bad = "a frame of no pixels";
    else if ((uint64_t)w * (uint64_t)h >= (1ull << 32)) bad = "a frame of 2^32 pixels or more";
    else if (!(P->rel_tol >= 0.0)) bad = "rel_tol negative or NaN";
    else if (!(P->lum_floor > 0.0)) bad = "lum_floor not above 0";
    if (bad) {
        set_error(std::string(name) + ": bad argument (" + bad + ")");
        return RT_ERR_ARG;
    }
    return RT_OK;
}

} // namespace

namespace rtc {

int select_begin(const char* name, size_t n_blocks, hipStream_t st, SelectPass& pass)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) {
        set_error(std::string(name) + ": device index out of range");
        return RT_ERR_ARG;
    }
    pass.lock = std::unique_lock<std::mutex>(g_scratch_mutex);
    SelectScratch& S = g_scratch[dev];
    pass.S = &S;
    if (!S.done) HIP_TRY(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    if (n_blocks > S.blocks) { // (hipFree waits for the device, so no queued pass still reads the old arrays)
        if (S.masks) (void)hipFree(S.masks);
        if (S.counts) (void)hipFree(S.counts);
        S.masks = nullptr;
        S.counts = nullptr;
        S.blocks = 0;
        HIP_TRY(hipMalloc(&S.masks, n_blocks * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc(&S.counts, n_blocks * sizeof(unsigned int)));
        S.blocks = n_blocks;
    }
    if (S.any && st != S.last) HIP_TRY(hipStreamWaitEvent(st, S.done, 0));
    return RT_OK;
}

void select_scan(SelectPass& pass, int n_blocks, unsigned int* d_total, hipStream_t st)
{
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, st, pass.S->counts, n_blocks, d_total);
}

int select_end(SelectPass& pass, hipStream_t st)
{
    SelectScratch& S = *pass.S;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S.done, st));
    S.last = st;
    S.any = true;
    return RT_OK;
}

} // namespace rtc

extern "C" {

int rt_adaptive_select_device(const rt_adaptive_params* P, const double* d_sum, const uint32_t* d_samples,
                              const uint32_t* d_misses, const double* d_q, const uint32_t* d_batches, uint64_t plane,
                              int32_t width, int32_t height, uint32_t* d_pixels, uint32_t cap, uint32_t* d_count, void* stream)
{
    int rc = check_select("rt_adaptive_select_device", P, d_sum, d_samples, d_misses, d_q, d_batches, width, height, d_pixels,
                          cap);
    if (rc != RT_OK) return rc;
    if (!d_count) {
        set_error("rt_adaptive_select_device: bad argument (null pointer)");
        return RT_ERR_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    SelectArgs A{*P, d_sum, d_samples, d_misses, d_q, d_batches, plane ? (size_t)plane : (size_t)width * (size_t)height,
                 width, height, (width + 7) / 8, 0};
    A.n_blocks = A.blocks_x * ((height + 7) / 8);
    SelectPass pass;
    rc = select_begin("rt_adaptive_select_device", (size_t)A.n_blocks, st, pass);
    if (rc != RT_OK) return rc;
    const unsigned grid = (unsigned)((A.n_blocks + 3) / 4);
    hipLaunchKernelGGL(adaptive_count_kernel, dim3(grid), dim3(256), 0, st, A, pass.S->masks, pass.S->counts);
    select_scan(pass, A.n_blocks, d_count, st);
    if (cap > 0)
        hipLaunchKernelGGL(adaptive_write_kernel, dim3(grid), dim3(256), 0, st, A, pass.S->masks, pass.S->counts, d_pixels, cap);
    return select_end(pass, st);
}

int64_t rt_debug_adaptive_select(const rt_adaptive_params* P, const double* sum, const uint32_t* samples, const uint32_t* misses,
                                 const double* q, const uint32_t* batches, uint64_t plane, int32_t width, int32_t height,
                                 uint32_t* pixels, uint32_t cap)
{
    const int rc = check_select("rt_debug_adaptive_select", P, sum, samples, misses, q, batches, width, height, pixels, cap);
    if (rc != RT_OK) return rc;
    const size_t pl = plane ? (size_t)plane : (size_t)width * (size_t)height;
    const int blocks_x = (width + 7) / 8, blocks_y = (height + 7) / 8;
    int64_t n = 0;
    for (int by = 0; by < blocks_y; by++)
        for (int bx = 0; bx < blocks_x; bx++)
            for (int l = 0; l < 64; l++) {
                const int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
                if (x >= width || y >= height) continue;
                const size_t a = (size_t)y * (size_t)width + (size_t)x;
                if (!adaptive_active(*P, sum[a], sum[pl + a], sum[2 * pl + a], samples[a], misses[a], q[a], batches[a])) continue;
                if (n < (int64_t)cap) pixels[n] = (uint32_t)a;
                n++;
            }
    return n;
}

} // extern "C"
