// kernels_fold.hip -- the kernels around the path launches that trace no ray: the folds of the path kernels'
// partials into fp64 accumulators (accumulate_*, per pixel, ray, list entry or probe), tonemap, the host
// layouts, the 1-spp colours, the pixel keys and the leaf compaction, each with its launcher.  Not a source
// of a scene-specialised build, and without rt_trace.h: nothing here changes a cached JIT kernel.
#include "../../include/rtcore_rng.h"
#include "rt_kernels.h"
#include "rt_surfel.h"
#include "rt_sh.h"
#include "rt_probe_error.h"

namespace rtc {
namespace {

// plane: element stride between the R, G and B planes of sum (>= w*h; a gather slot may be taller
// than the band set written into it).  set_rays (an overlapped launch, run_path): the launch set's own
// ray counter, which the path kernel added into; one thread moves it into the caller's and zeroes it, so
// the caller's counter changes in its stream's order and the path kernel touches no caller memory.
__global__ void accumulate_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, size_t plane,
                                  unsigned long long* set_rays, unsigned long long* rays)
{
    if (set_rays && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        atomicAdd(rays, *set_rays);
        *set_rays = 0;
    }
    const int x = blockIdx.x * 16 + (threadIdx.x & 15);
    const int y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= p.w || y >= p.h) return;
    size_t blk = (size_t)((y >> 3) * p.blocks_x + (x >> 3));
    const int q = (y & 7) * 8 + (x & 7);
    const size_t i = (size_t)y * p.w + x;
    if (p.cull) { // a launch over the live blocks: a dead block's pixels are spp primary misses, their sums stay
        const int live = (int)p.cull[kCullTable + (p.n_pad >> 6) + blk];
        if (live < 0) {
            misses[i] += (uint32_t)p.spp;
            return;
        }
        blk = (size_t)live;
    }
    double r = sum[i], g = sum[plane + i], bl = sum[2 * plane + i];
    uint32_t ns = 0, nm = 0;
    const int used = (p.spp + p.chunk - 1) / p.chunk; // chunks past spp hold no partial
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[(((blk << p.log2_chunks) + c) << 6) + q];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
    }
    sum[i] = r;
    sum[plane + i] = g;
    sum[2 * plane + i] = bl;
    samples[i] += ns;
    misses[i] += nm;
}

// rt_render_rays: the same fold per ray (ray i's partials are pixel i & 63 of block i >> 6), in chunk
// order.  recs null: added to the planar accumulators (n each, planes n apart); else written, from
// zero, as one TileRec per ray for the host entry's download.
__global__ void accumulate_rays_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, TileRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = p.n_rays;
    if (i >= n) return;
    double r = 0.0, g = 0.0, bl = 0.0;
    if (!recs) {
        r = sum[i];
        g = sum[n + i];
        bl = sum[2 * n + i];
    }
    uint32_t ns = 0, nm = 0;
    const int used = (p.spp + p.chunk - 1) / p.chunk;
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[((((i >> 6) << p.log2_chunks) + c) << 6) + (i & 63)];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
    }
    if (recs) {
        TileRec t;
        t.r = r;
        t.g = g;
        t.b = bl;
        t.samples = ns;
        t.misses = nm;
        recs[i] = t;
    } else {
        sum[i] = r;
        sum[n + i] = g;
        sum[2 * n + i] = bl;
        samples[i] += ns;
        misses[i] += nm;
    }
}

// rt_render_pixels: the fold per list entry.  Entry i's partials are at accumulate_rays_kernel's
// addresses; they go, in chunk order, into the frame accumulators at the entry's pixel a = pix (row-major
// y * W + x is the list's own index), exactly as accumulate_kernel adds a window's: r = sum[a], then
// r += v.x per chunk.  With q: per used chunk j of t_j = samples + misses > 0 finished samples,
// Y_j = 0.299 r + 0.587 g + 0.114 b of the chunk's fp32 sums (DoubleColor.GetLuminance, left to
// right, every operation rounded on its own), q += Y_j Y_j / t_j and batches += 1.  recs: the same
// from zero as one PixelRec per entry (the host entry's download), zero for a skipped entry.
// (fold_entry: entry i's partials into the accumulators at a; rt_render_list's fold below is the same.)
__device__ __forceinline__ void fold_entry(const PathParams& p, size_t i, size_t a, bool inside, double* sum,
                                           uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches, size_t plane,
                                           PixelRec* recs)
{
    if (!inside && !recs) return;
    double r = 0.0, g = 0.0, bl = 0.0, qs = 0.0;
    if (!recs) {
        r = sum[a];
        g = sum[plane + a];
        bl = sum[2 * plane + a];
    }
    uint32_t ns = 0, nm = 0, nb = 0;
    const int used = inside ? (p.spp + p.chunk - 1) / p.chunk : 0;
    for (int c = 0; c < used; c++) {
        const float4 v = p.partial[((((i >> 6) << p.log2_chunks) + c) << 6) + (i & 63)];
        r += v.x;
        g += v.y;
        bl += v.z;
        const uint32_t k = __float_as_uint(v.w);
        ns += k & 0xFFFFu;
        nm += k >> 16;
        const uint32_t t = (k & 0xFFFFu) + (k >> 16);
        if ((q || recs) && t > 0) {
            const double y = __dadd_rn(__dadd_rn(__dmul_rn(0.299, (double)v.x), __dmul_rn(0.587, (double)v.y)),
                                       __dmul_rn(0.114, (double)v.z));
            qs = __dadd_rn(qs, __ddiv_rn(__dmul_rn(y, y), (double)t));
            nb++;
        }
    }
    if (recs) {
        PixelRec t;
        t.r = r;
        t.g = g;
        t.b = bl;
        t.q = qs;
        t.samples = ns;
        t.misses = nm;
        t.batches = nb;
        t.pad = 0;
        recs[i] = t;
    } else {
        sum[a] = r;
        sum[plane + a] = g;
        sum[2 * plane + a] = bl;
        samples[a] += ns;
        misses[a] += nm;
        if (q) {
            q[a] = __dadd_rn(q[a], qs);
            batches[a] += nb;
        }
    }
}

__global__ void accumulate_pixels_kernel(PathParams p, double* sum, uint32_t* samples, uint32_t* misses, double* q,
                                         uint32_t* batches, size_t plane, PixelRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t a = p.pixel_list[i];
    fold_entry(p, i, a, a < (size_t)p.n_frame_px, sum, samples, misses, q, batches, plane, recs);
}

// rt_render_list: accumulate_pixels_kernel for a RAYS, BEAMS or SURFELS launch.  List position i's partials
// go into the per-entry accumulators at e = index[i] (i itself without a list, where the sums are
// accumulate_rays_kernel's: r = sum[e], then r += v.x per chunk), an entry at or past n_records is
// skipped; recs: one PixelRec per list position, from zero.
__global__ void accumulate_list_kernel(PathParams p, const uint32_t* index, size_t n_records, double* sum, uint32_t* samples,
                                       uint32_t* misses, double* q, uint32_t* batches, size_t plane, PixelRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t e = index ? (size_t)index[i] : i;
    fold_entry(p, i, e, e < n_records, sum, samples, misses, q, batches, plane, recs);
}

// rt_render_probes: the fold of a SURFELS launch in RT_GATHER_SPHERE with one sample per work item
// (make_params_probes), one thread per probe as accumulate_rays_kernel, so that a wave's loads of chunk k
// are 64 consecutive float4.  Row k of probe i is sample k's fp32 colour and its hit or miss; the sample's
// direction is drawn again as the launch drew it (refill: the stream's first two draws through
// surfel_sample) and weighs the colour, or for a primary miss the count, by the nine basis functions of
// rt_sh.h: fp64, product and sum each rounded on its own, in sample order from what the accumulators hold.
// recs null: sh, samples and misses of the probe; else recs[i], which came up with the caller's sums and
// zero counts and goes down to the host entry.  The 36 sums stay in registers; no LDS, no atomics.
// (fold_probe: list position i's partials into the accumulators of entry e; the two kernels below.)
// LIST (rt_render_probe_list): the record, the stream's key and the accumulators are entry e's, the partials
// list position i's.  MOM: the entry's rt_probe_moments (rt_probe_error.h) as eight more sums in registers.
template <bool LIST, bool MOM>
__device__ __forceinline__ void fold_probe(const PathParams& p, size_t i, size_t e, rt_probe_sh* sh, uint32_t* samples,
                                           uint32_t* misses, ProbeRec* recs, rt_probe_moments* mom)
{
    double* const acc = !LIST && recs ? &recs[e].sh.c[0][0] : &sh[e].c[0][0];
    double c[kShCoeffs][4];
#pragma unroll
    for (int l = 0; l < kShCoeffs; l++)
#pragma unroll
        for (int j = 0; j < 4; j++) c[l][j] = acc[4 * l + j];
    [[maybe_unused]] double m0[kProbeMomentRows], m1[kProbeMomentRows];
    if constexpr (MOM) {
#pragma unroll
        for (int l = 0; l < kProbeMomentRows; l++) {
            m0[l] = mom[e].m[l][0];
            m1[l] = mom[e].m[l][1];
        }
    }
    uint32_t ns = 0, nm = 0;
    const double2* const rows = p.ray_list + 4 * e;
    const rt_key2 pkey = rt_rng_pixel_key(p.seed_key, p.stream_base + (unsigned long long)e);
    const float4* const row = p.partial + ((((i >> 6) << p.log2_chunks) << 6) + (i & 63));
    for (int k = 0; k < p.spp; k++) { // (chunk == 1: chunk k is sample k)
        const float4 v = row[(size_t)k << 6];
        const uint32_t w = __float_as_uint(v.w);
        rt_rng rng = rt_rng_from_pixel_key(pkey, p.sample_base + (unsigned long long)k);
        const float u1 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        const float u2 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        V3 o, d;
        if (!surfel_sample(rows, RT_GATHER_SPHERE, u1, u2, o, d)) { // an invalid probe: a miss in no direction
            nm++;
            continue;
        }
        double Y[kShCoeffs];
        sh_basis((double)d.x, (double)d.y, (double)d.z, Y);
        if (w >> 16) {
            nm++;
#pragma unroll
            for (int l = 0; l < kShCoeffs; l++) c[l][3] = __dadd_rn(c[l][3], Y[l]);
            if constexpr (MOM) probe_moments_miss(m1, Y);
        } else if (w & 0xFFFFu) {
            ns++;
            const double r = (double)v.x, g = (double)v.y, b = (double)v.z;
#pragma unroll
            for (int l = 0; l < kShCoeffs; l++) {
                c[l][0] = __dadd_rn(c[l][0], __dmul_rn(r, Y[l]));
                c[l][1] = __dadd_rn(c[l][1], __dmul_rn(g, Y[l]));
                c[l][2] = __dadd_rn(c[l][2], __dmul_rn(b, Y[l]));
            }
            if constexpr (MOM) probe_moments_hit(m0, v.x, v.y, v.z, Y);
        }
    }
#pragma unroll
    for (int l = 0; l < kShCoeffs; l++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[4 * l + j] = c[l][j];
    if constexpr (MOM) {
#pragma unroll
        for (int l = 0; l < kProbeMomentRows; l++) {
            mom[e].m[l][0] = m0[l];
            mom[e].m[l][1] = m1[l];
        }
    }
    if (!LIST && recs) {
        recs[e].samples += ns;
        recs[e].misses += nm;
    } else {
        samples[e] += ns;
        misses[e] += nm;
    }
}

__global__ void __launch_bounds__(256) accumulate_probes_kernel(PathParams p, rt_probe_sh* sh, uint32_t* samples,
                                                                uint32_t* misses, ProbeRec* recs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    fold_probe<false, false>(p, i, i, sh, samples, misses, recs, nullptr);
}

// rt_render_probe_list: the same fold for a launch with an index list (run_rays, records not gathered): list
// position i's rows are samples of entry e = index[i] (null: i), whose record, stream and accumulators they
// go with; an entry at or past n_records opened no item and is skipped.  mom (MOM): the entry's moments.
template <bool MOM>
__global__ void __launch_bounds__(256) accumulate_probe_list_kernel(PathParams p, const uint32_t* index, size_t n_records,
                                                                    rt_probe_sh* sh, uint32_t* samples, uint32_t* misses,
                                                                    rt_probe_moments* mom)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.n_rays) return;
    const size_t e = index ? (size_t)index[i] : i;
    if (e >= n_records) return;
    fold_probe<true, MOM>(p, i, e, sh, samples, misses, nullptr, mom);
}

// SampleSet.GetOutput / GetColorCode (SampleSet.cs:50-113) per pixel of planar accumulators.
__device__ __forceinline__ uint32_t color_code(double r, double g, double b, double a)
{
    auto q = [](double v) { // Util.Clamp to [0, 1], then (int)(v * 255)
        v = v > 0.0 ? v : 0.0;
        v = v < 1.0 ? v : 1.0;
        return (uint32_t)(int32_t)(v * 255);
    };
    return (q(a) << 24) | (q(r) << 16) | (q(g) << 8) | q(b);
}

__global__ void tonemap_kernel(int w, int h, const double* __restrict__ sum, const uint32_t* __restrict__ samples,
                               const uint32_t* __restrict__ misses, double br, double bg, double bb, double back_alpha,
                               double exposure, int32_t* __restrict__ argb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = w * h;
    if (i >= n) return;
    const uint32_t ns = samples[i], nm = misses[i];
    if (ns == 0) {
        argb[i] = (int32_t)color_code(br * exposure, bg * exposure, bb * exposure, back_alpha);
        return;
    }
    const double total = (double)ns + (double)nm;
    const double mult = exposure / ns;
    double r = sum[i] * mult, g = sum[n + i] * mult, b = sum[2 * (size_t)n + i] * mult, a = 1;
    const double bam = nm / total, bk = bam * back_alpha;
    r += (br - r) * bk;
    g += (bg - g) * bk;
    b += (bb - b) * bk;
    a += (back_alpha - a) * bam;
    const double gamma = 1 / 2.2;
    argb[i] = (int32_t)color_code(pow(r, gamma), pow(g, gamma), pow(b, gamma), a);
}

// One pass of Raytracer.Render (1 spp): DoubleColor[w, h] with Placeholder (-1) on a primary miss,
// in the caller's order x * h + y, as fp32 -- a sample's colour is fp32 in the kernel, so the host
// widens it to double exactly, and the PCIe copy is 12 B per pixel instead of 24.
__global__ void colors_1spp_kernel(PathParams p, float* __restrict__ out)
{
    const size_t npix = (size_t)p.w * p.h;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const int x = (int)(o / (size_t)p.h), y = (int)(o - (size_t)x * p.h);
    int blk = (y >> 3) * p.blocks_x + (x >> 3);
    if (p.cull) blk = (int)p.cull[kCullTable + (p.n_pad >> 6) + blk]; // live number, or -1: a dead block, a miss
    const int q = (blk < 0 ? 0 : blk) * 64 + (y & 7) * 8 + (x & 7); // 1 spp: one chunk
    const float4 v = blk < 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : p.partial[q];
    const bool miss = (__float_as_uint(v.w) & 0xFFFFu) == 0;
    out[3 * o + 0] = miss ? -1.0f : v.x;
    out[3 * o + 1] = miss ? -1.0f : v.y;
    out[3 * o + 2] = miss ? -1.0f : v.z;
}

// rt_trace_paths: the records and per-sample rows of a launch, which the path kernel wrote row-major
// over the tile (sample (py * w + px) * spp + k), into the caller's order (x * h + y) * spp + k.
// One thread per 16-byte row: rows = kRecRows * (recursion + 1) per sample of `rays`, 1 of `samples`.
__global__ void trace_host_layout_kernel(int w, int h, int spp, int rows, const float4* __restrict__ rays,
                                         const float4* __restrict__ samples, float4* __restrict__ rays_out,
                                         float4* __restrict__ samples_out)
{
    const size_t n = (size_t)w * h * spp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (size_t)(rows + 1)) return;
    const size_t so = i / (size_t)(rows + 1), row = i - so * (size_t)(rows + 1); // the caller's sample, its row
    const size_t pix = so / (size_t)spp, k = so - pix * (size_t)spp;
    const size_t x = pix / (size_t)h, y = pix - x * (size_t)h;
    const size_t si = (y * (size_t)w + x) * (size_t)spp + k;
    if (row < (size_t)rows) rays_out[so * rows + row] = rays[si * rows + row];
    else samples_out[so] = samples[si];
}

// Planar row-major tile accumulators -> the caller's SampleSet order (C# [x, y]: x * h + y), one
// 32-B record per pixel (DoubleColor, samples, misses), so that the host-buffer entry point copies
// one contiguous image in chunks and adds each chunk sequentially as it lands.
__global__ void tile_host_layout_kernel(int w, int h, const double* __restrict__ sum, const uint32_t* __restrict__ ns,
                                        const uint32_t* __restrict__ ms, TileRec* __restrict__ out)
{
    const size_t npix = (size_t)w * h;
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix) return;
    const size_t x = o / (size_t)h, y = o - x * (size_t)h;
    const size_t i = y * (size_t)w + x;
    TileRec r;
    r.r = sum[i];
    r.g = sum[npix + i];
    r.b = sum[2 * npix + i];
    r.samples = ns[i];
    r.misses = ms[i];
    out[o] = r;
}

// ---- compact leaves (rt_internal.h): 48-B rows and homogeneous leaf references --------------
__global__ void rows_kernel(const TestRec* __restrict__ tests, int n, float4* __restrict__ rows)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const TestRec t = tests[i];
    rows[3 * (size_t)i] = t.r0;
    rows[3 * (size_t)i + 1] = t.r1;
    rows[3 * (size_t)i + 2] = t.r2;
}

// A generic leaf whose primitives (at most 4, all of them at slots below 2^23) share their kind
// (triangle or sphere) and test flags becomes a compact leaf; any other reference is returned
// unchanged.  (A leaf reaching past slot 2^23 stays generic: leaf_advance adds to the first-slot
// field, whose carry would run into the flag bits.)
__device__ int compact_ref(int ref, const TestRec* __restrict__ tests)
{
    if (ref >= 0 || ref == RT_NODE4_EMPTY) return ref;
    const int code = ~ref;
    if (code & kLeafCompact) return ref;
    const int first = code >> 3, count = (code & 7) + 1;
    if (count > 4 || first + count > kLeafCompactMaxFirst) return ref;
    uint32_t key = 0;
    for (int j = 0; j < count; j++) {
        const uint32_t fl = __float_as_uint(tests[first + j].meta.y), kind = fl & KIND_MASK;
        if (kind != RT_PRIM_TRIANGLE && kind != RT_PRIM_SPHERE) return ref;
        const uint32_t lf = (kind == RT_PRIM_SPHERE ? 1u : 0u) | ((fl >> 1) & 0xEu) | ((fl >> 2) & 0x10u);
        if (j > 0 && lf != key) return ref;
        key = lf;
    }
    return ~(kLeafCompact | (int)(key << 25) | (first << 2) | (count - 1));
}

__global__ void compact_nodes_kernel(NodeF* __restrict__ n2, int n_n2, Node4Q* __restrict__ n4, int n_n4,
                                     const TestRec* __restrict__ tests)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_n2) {
        NodeF& n = n2[i];
        n.lmin.w = __int_as_float(compact_ref(__float_as_int(n.lmin.w), tests));
        n.rmin.w = __int_as_float(compact_ref(__float_as_int(n.rmin.w), tests));
    }
    if (i < n_n4) {
        Node4Q& q = n4[i];
        q.c.z = __int_as_float(compact_ref(__float_as_int(q.c.z), tests));
        q.c.w = __int_as_float(compact_ref(__float_as_int(q.c.w), tests));
        q.d.x = __int_as_float(compact_ref(__float_as_int(q.d.x), tests));
        q.d.y = __int_as_float(compact_ref(__float_as_int(q.d.y), tests));
    }
}
} // namespace

hipError_t launch_accumulate(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses, hipStream_t stream,
                             size_t plane, unsigned long long* d_set_rays, unsigned long long* d_rays)
{
    if (plane == 0) plane = (size_t)p.w * p.h;
    dim3 grid((p.w + 15) / 16, (p.h + 15) / 16);
    hipLaunchKernelGGL(accumulate_kernel, grid, dim3(256), 0, stream, p, d_sum, d_samples, d_misses, plane, d_set_rays,
                       d_rays);
    return hipGetLastError();
}

hipError_t launch_accumulate_rays(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                  TileRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_rays_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sum, d_samples,
                       d_misses, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_pixels(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                    double* d_q, uint32_t* d_batches, size_t plane, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    if (plane == 0) plane = (size_t)p.n_frame_px;
    hipLaunchKernelGGL(accumulate_pixels_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sum, d_samples,
                       d_misses, d_q, d_batches, plane, (PixelRec*)nullptr);
    return hipGetLastError();
}

hipError_t launch_accumulate_list(const PathParams& p, const uint32_t* d_index, size_t n_records, double* d_sum,
                                  uint32_t* d_samples, uint32_t* d_misses, double* d_q, uint32_t* d_batches, size_t plane,
                                  PixelRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    if (plane == 0) plane = n_records;
    hipLaunchKernelGGL(accumulate_list_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_index, n_records,
                       d_sum, d_samples, d_misses, d_q, d_batches, plane, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_probes(const PathParams& p, rt_probe_sh* d_sh, uint32_t* d_samples, uint32_t* d_misses,
                                    ProbeRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_probes_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, d_sh, d_samples,
                       d_misses, d_recs);
    return hipGetLastError();
}

hipError_t launch_accumulate_probe_list(const PathParams& p, const uint32_t* d_index, size_t n_records, rt_probe_sh* d_sh,
                                        uint32_t* d_samples, uint32_t* d_misses, rt_probe_moments* d_moments,
                                        hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    const dim3 grid((p.n_rays + 255u) / 256u);
    if (d_moments)
        hipLaunchKernelGGL(accumulate_probe_list_kernel<true>, grid, dim3(256), 0, stream, p, d_index, n_records, d_sh,
                           d_samples, d_misses, d_moments);
    else
        hipLaunchKernelGGL(accumulate_probe_list_kernel<false>, grid, dim3(256), 0, stream, p, d_index, n_records, d_sh,
                           d_samples, d_misses, d_moments);
    return hipGetLastError();
}

hipError_t launch_accumulate_pixels_recs(const PathParams& p, PixelRec* d_recs, hipStream_t stream)
{
    if (p.n_rays == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_pixels_kernel, dim3((p.n_rays + 255u) / 256u), dim3(256), 0, stream, p, (double*)nullptr,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, (double*)nullptr, (uint32_t*)nullptr, (size_t)0, d_recs);
    return hipGetLastError();
}

hipError_t launch_tonemap(int w, int h, const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses,
                          rt_color back, double back_alpha, double exposure, int32_t* d_argb, hipStream_t stream)
{
    const int n = w * h;
    hipLaunchKernelGGL(tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, w, h, d_sum, d_samples, d_misses,
                       back.r, back.g, back.b, back_alpha, exposure, d_argb);
    return hipGetLastError();
}

hipError_t launch_tile_host_layout(int w, int h, const double* d_sum, const uint32_t* d_samples,
                                  const uint32_t* d_misses, TileRec* d_out, hipStream_t stream)
{
    const size_t npix = (size_t)w * h;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(tile_host_layout_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, w, h, d_sum,
                       d_samples, d_misses, d_out);
    return hipGetLastError();
}

hipError_t launch_trace_host_layout(int w, int h, int spp, int recursion, const float4* d_rays, const float4* d_samples,
                                    float4* d_rays_out, float4* d_samples_out, hipStream_t stream)
{
    const int rows = kRecRows * (recursion + 1);
    const size_t n = (size_t)w * h * spp * (size_t)(rows + 1);
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(trace_host_layout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, h, spp, rows,
                       d_rays, d_samples, d_rays_out, d_samples_out);
    return hipGetLastError();
}

hipError_t compact_leaves(const TestRec* d_tests, int n_records, float4* d_rows, NodeF* d_nodes, int n_nodes,
                          Node4Q* d_nodes4, int n_nodes4, bool rewrite, hipStream_t stream)
{
    if (n_records > 0)
        hipLaunchKernelGGL(rows_kernel, dim3((n_records + 255) / 256), dim3(256), 0, stream, d_tests, n_records, d_rows);
    const int n = std::max(n_nodes, n_nodes4);
    if (rewrite && n > 0)
        hipLaunchKernelGGL(compact_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_nodes, n_nodes, d_nodes4,
                           n_nodes4, d_tests);
    return hipGetLastError();
}

__global__ void pixel_keys_kernel(rt_key2 seed_key, int w, int h, rt_key2* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)w * (size_t)h) return;
    out[i] = rt_rng_pixel_key(seed_key, (unsigned long long)i);
}

hipError_t launch_pixel_keys(rt_key2 seed_key, int w, int h, rt_key2* out, hipStream_t stream)
{
    const size_t n = (size_t)w * (size_t)h;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pixel_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed_key, w, h, out);
    return hipGetLastError();
}

hipError_t launch_colors_1spp(const PathParams& p, float* d_out, hipStream_t stream)
{
    const size_t npix = (size_t)p.w * p.h;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(colors_1spp_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, p, d_out);
    return hipGetLastError();
}

} // namespace rtc
