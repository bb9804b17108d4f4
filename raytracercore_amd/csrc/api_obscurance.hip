// api_obscurance.hip -- the C ABI's obscurance at surfels (include/rtcore.h, "obscurance at surfels",
// rt_obscurance): per surface point the sums of its gather samples' falloff weights, of their squares and of
// the unoccluded directions (the bent normal), and the selection pass that turns those into the next list of an
// adaptive bake.  The fold kernels (two layouts), the selection kernels and the host twins are compilations of
// rt_obscurance.h.  A chunk is three launches: the listed entries' sample rays into the scene's scratch (a
// compilation of rt_surfel.h's surfel_sample that reads the list), rt_query_rays_device's closest-hit launch
// (launch_rays, api_query.hip) over those rays, and the fold.  The selection pass needs no scene and shares
// rt_adaptive_select_device's scan and scratch (select_scan.h).
#include <cstdlib>
#include <cstring>
#include <limits>

#include "rt_obscurance.h"
#include "rt_scene.h"
#include "rt_surfel.h"
#include "select_scan.h"

static_assert(sizeof(rt_obscurance_params) == 24 && sizeof(rt_obscurance) == 48 && sizeof(rt_obscurance_select_params) == 16,
              "rtcore.h: obscurance at surfels");
static_assert(offsetof(rt_obscurance, samples) == 40 && offsetof(rt_obscurance, hits) == 44, "rt_obscurance: five doubles, two counts");
static_assert(sizeof(rt_hit) == 48 && sizeof(rt_ray) == 64, "the scratch: 64 + 48 B per sample");

namespace {

constexpr int32_t kObscuranceMaxSpp = 1 << 19; // one entry's samples are one chunk at the most
constexpr int kFoldWaves = 4;                  // entries per block of the wave-per-entry fold

bool known_mode(int32_t mode) { return mode == RT_GATHER_DIFFUSE || mode == RT_GATHER_COSINE || mode == RT_GATHER_SPHERE; }

// surfel_rays_kernel (api_render_surfels.hip) for list positions: sample `at` belongs to position at / spp,
// whose entry is index[position] (index null: first + position); the draws are keyed by the entry.  An entry
// at or past n_records gets all-zero rays, as an invalid surfel does.
__global__ void __launch_bounds__(256) obscurance_rays_kernel(const double2* __restrict__ surfels, const uint32_t* __restrict__ index,
                                                              unsigned first, unsigned n_records, unsigned total, unsigned spp, int mode,
                                                              rt_key2 seed_key, unsigned long long sample_base,
                                                              unsigned long long stream_base, double2* __restrict__ out)
{
    const unsigned at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const unsigned j = at / spp, k = at - j * spp;
    const unsigned e = index ? index[j] : first + j;
    double2* const row = out + 4 * (size_t)at;
    V3 o, d;
    bool ok = false;
    if (e < n_records) {
        rt_rng rng = rt_rng_from_pixel_key(rt_rng_pixel_key(seed_key, stream_base + e), sample_base + k);
        const float u1 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        const float u2 = (float)rt_rng_next24(&rng) * 0x1p-24f;
        ok = surfel_sample(surfels + 4 * (size_t)e, mode, u1, u2, o, d);
    }
    if (ok) {
        row[0] = make_double2((double)o.x, (double)o.y);
        row[1] = make_double2((double)o.z, 1.0);
        row[2] = make_double2((double)d.x, (double)d.y);
        row[3] = make_double2((double)d.z, 0.0);
    } else {
        row[0] = row[1] = row[2] = row[3] = make_double2(0.0, 0.0);
    }
}

struct FoldArgs {
    const rt_ray* rays;
    const rt_hit* hits;
    const uint32_t* index; // the chunk's list positions, or null: entries first + position
    unsigned first, n_records, n, spp;
    double radius;
    int power;
    rt_obscurance* acc; // indexed by entry
};

// Layout (b), one wave per list position.  The five values a sample adds are free of order: the 64 lanes take
// 64 consecutive samples, read their direction and hit coalesced, and leave the values in the wave's LDS rows,
// five doubles per sample.  The sums are not: lanes 0 .. 4 own one sum each and add the batch's values in
// sample order (an odd stride of doubles: the five lanes read five banks).  The samples of an invalid surfel add
// nothing, not even a zero, so the batch's valid lanes travel as a ballot mask.  The LDS rows are a wave's own
// and the position is wave-uniform (readfirstlane), so no barrier between waves is needed.
__global__ void __launch_bounds__(64 * kFoldWaves) obscurance_fold_wave_kernel(FoldArgs A)
{
    __shared__ double terms[kFoldWaves][64 * kObscuranceTerms];
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned j = blockIdx.x * (unsigned)kFoldWaves + wave;
    if (j >= A.n) return;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)(A.index ? A.index[j] : A.first + j));
    if (e >= A.n_records) return;
    double* const mine = terms[wave];
    double* const rec = reinterpret_cast<double*>(A.acc + e);
    double sum = lane < (unsigned)kObscuranceTerms ? rec[lane] : 0.0;
    unsigned n_hits = 0;
    const rt_ray* __restrict__ r = A.rays + (size_t)j * A.spp;
    const rt_hit* __restrict__ h = A.hits + (size_t)j * A.spp;
    for (unsigned base = 0; base < A.spp; base += 64u) {
        const unsigned cnt = A.spp - base < 64u ? A.spp - base : 64u;
        bool valid = false, within = false;
        if (lane < cnt) {
            const unsigned k = base + lane;
            const double x = r[k].direction.x, y = r[k].direction.y, z = r[k].direction.z;
            valid = !obscurance_skipped(x, y, z);
            if (valid) {
                const double w = obscurance_weight(h[k].prim_id, h[k].distance, A.radius, A.power, within);
                double t[kObscuranceTerms];
                obscurance_terms(w, x, y, z, t);
#pragma unroll
                for (int a = 0; a < kObscuranceTerms; a++) mine[lane * kObscuranceTerms + a] = t[a];
            }
        }
        const unsigned long long mask = __ballot(valid);
        n_hits += (unsigned)__popcll(__ballot(valid && within));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < (unsigned)kObscuranceTerms)
            for (unsigned k = 0; k < cnt; k++)
                if ((mask >> k) & 1ull) sum = sh_add(sum, mine[k * kObscuranceTerms + lane]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < (unsigned)kObscuranceTerms) rec[lane] = sum;
    if (lane == 0) {
        A.acc[e].samples += A.spp;
        A.acc[e].hits += n_hits;
    }
}

// Layout (a), one thread per list position walking its samples' rows: the host twin's loop.
__global__ void __launch_bounds__(64) obscurance_fold_thread_kernel(FoldArgs A)
{
    const unsigned j = blockIdx.x * 64u + threadIdx.x;
    if (j >= A.n) return;
    const unsigned e = A.index ? A.index[j] : A.first + j;
    if (e >= A.n_records) return;
    rt_obscurance acc = A.acc[e];
    double sum[kObscuranceTerms] = {acc.o, acc.o2, acc.bent[0], acc.bent[1], acc.bent[2]};
    const rt_ray* __restrict__ r = A.rays + (size_t)j * A.spp;
    const rt_hit* __restrict__ h = A.hits + (size_t)j * A.spp;
    for (unsigned k = 0; k < A.spp; k++)
        obscurance_add(A.radius, A.power, r[k].direction.x, r[k].direction.y, r[k].direction.z, h[k].prim_id, h[k].distance, sum,
                       acc.samples, acc.hits);
    acc.o = sum[0];
    acc.o2 = sum[1];
    acc.bent[0] = sum[2];
    acc.bent[1] = sum[3];
    acc.bent[2] = sum[4];
    A.acc[e] = acc;
}

struct SelectArgs {
    rt_obscurance_select_params P;
    const rt_obscurance* acc;
    unsigned n_records;
    int n_blocks;
};

// probe_count_kernel's shape (api_probe_list.hip): one wave per 64 consecutive entries, four per workgroup; the
// block's active lanes as a ballot mask, and their number.
__global__ void __launch_bounds__(256) obscurance_count_kernel(SelectArgs A, unsigned long long* masks, unsigned int* counts)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= A.n_blocks) return; // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const unsigned e = (unsigned)b * 64u + (unsigned)lane; // (n_records < 2^32, so b < 2^26: no wrap)
    bool act = false;
    if (e < A.n_records) act = obscurance_active(A.P, A.acc[e].o, A.acc[e].o2, A.acc[e].samples);
    const unsigned long long m = __ballot(act);
    if (lane == 0) {
        masks[b] = m;
        counts[b] = (unsigned)__popcll(m);
    }
}

// The write: block b's active entries, in lane order, at offs[b] + the lane's rank in the mask; entries at or
// past cap are dropped.
__global__ void __launch_bounds__(256) obscurance_write_kernel(int n_blocks, const unsigned long long* masks, const unsigned int* offs,
                                                               uint32_t* list, uint32_t cap)
{
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long m = masks[b];
    if (!((m >> lane) & 1ull)) return;
    const unsigned int at = offs[b] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (at >= cap) return;
    list[at] = (uint32_t)b * 64u + (uint32_t)lane;
}

int bad_argument(const char* name, const char* what)
{
    set_error(std::string(name) + ": bad argument (" + what + ")");
    return RT_ERR_ARG;
}

// Samples of one chunk: kQueryChunk (RTCORE_QUERY_CHUNK), as every chunked query entry.
int64_t chunk_samples()
{
    int64_t chunk = kQueryChunk;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(kQueryChunk, atoll(e)));
    return chunk;
}

// The fold's layout: the wave-per-entry kernel, or with RTCORE_OBSCURANCE_FOLD=thread the thread-per-entry one
// (for A/B; both give the twin's bits).
bool fold_by_thread()
{
    const char* e = getenv("RTCORE_OBSCURANCE_FOLD");
    return e && !strcmp(e, "thread");
}

int check_select(const char* name, const rt_obscurance_select_params* P, const void* acc, int64_t n_records, const void* list,
                 uint32_t cap)
{
    const char* bad = nullptr;
    if (!P || !acc || (!list && cap > 0)) bad = "null pointer";
    else if (n_records <= 0) bad = "n_records <= 0";
    else if (n_records >= ((int64_t)1 << 32)) bad = "2^32 entries or more";
    else if (!(P->tol >= 0.0)) bad = "tol negative or NaN";
    return bad ? bad_argument(name, bad) : RT_OK;
}

} // namespace

extern "C" {

int rt_obscurance_surfels_device(rt_scene* s, int32_t gather_mode, const rt_surfel* d_surfels, int64_t n_records,
                                 const uint32_t* d_index, int64_t n, const rt_obscurance_params* params, int32_t spp, uint64_t seed,
                                 uint64_t sample_base, uint64_t stream_base, rt_obscurance* d_acc, void* stream)
{
    const char* name = "rt_obscurance_surfels_device";
    const char* bad = !known_mode(gather_mode) ? "unknown gather mode" : !s ? "null scene" : n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) return RT_OK;
    if (!bad)
        bad = (!d_surfels || !d_acc || !params)         ? "null pointer"
              : (n_records <= 0 || n_records >> 32)     ? "n_records <= 0 or >= 2^32"
              : (!d_index && n != n_records)            ? "no index list and n != n_records"
              : !obscurance_params_ok(params)           ? kObscuranceParamsRule
              : spp > kObscuranceMaxSpp                 ? "spp above 2^19: split the call by sample_base"
                                                        : nullptr;
    if (bad) return bad_argument(name, bad);
    if (s->resolved == RT_TRAVERSAL_BVH2) {
        set_error(std::string(name) + ": runs rt_query_rays' RT_QUERY_FAST kernels (traversal modes BRUTE, GROUPED and BVH); this "
                                      "scene is in BVH2 mode (rt_scene_set_traversal), use RT_TRAVERSAL_BVH");
        return RT_ERR_STATE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t positions = std::min<int64_t>(n, std::max<int64_t>(1, chunk_samples() / spp)); // a chunk holds whole positions
    const bool by_thread = fold_by_thread();
    const rt_key2 seed_key = rt_rng_seed_key(seed);
    HIP_TRY(hipSetDevice(s->device));
    // (the depth bake's scratch: both are one chunk's sample rays and their closest hits)
    HIP_TRY(s->probe_depth_rays.reserve((size_t)positions * (size_t)spp));
    HIP_TRY(s->probe_depth_hits.reserve((size_t)positions * (size_t)spp));
    // the rays, their hits, the work counter and the stack overflow area are the scene's: order after its last operation
    HIP_TRY(wait_last_op(s, st));
    for (int64_t a = 0; a < n; a += positions) {
        const unsigned m = (unsigned)std::min(positions, n - a);
        const unsigned total = m * (unsigned)spp; // (at most 2^19)
        const uint32_t* index = d_index ? d_index + a : nullptr;
        hipLaunchKernelGGL(obscurance_rays_kernel, dim3((total + 255u) / 256u), dim3(256), 0, st,
                           reinterpret_cast<const double2*>(d_surfels), index, (unsigned)a, (unsigned)n_records, total, (unsigned)spp,
                           gather_mode, seed_key, (unsigned long long)sample_base, (unsigned long long)stream_base,
                           reinterpret_cast<double2*>(s->probe_depth_rays.p));
        HIP_TRY(hipGetLastError());
        const int rc = launch_rays(s, RT_QUERY_FAST, s->probe_depth_rays.p, total, s->probe_depth_hits.p, st);
        if (rc != RT_OK) return rc;
        const FoldArgs A{s->probe_depth_rays.p, s->probe_depth_hits.p, index, (unsigned)a, (unsigned)n_records, m, (unsigned)spp,
                         params->radius, params->power, d_acc};
        if (by_thread) hipLaunchKernelGGL(obscurance_fold_thread_kernel, dim3((m + 63u) / 64u), dim3(64), 0, st, A);
        else hipLaunchKernelGGL(obscurance_fold_wave_kernel, dim3((m + kFoldWaves - 1) / kFoldWaves), dim3(64 * kFoldWaves), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return end_op(s, st);
}

int rt_debug_obscurance_fold(const rt_obscurance_params* params, const rt_ray* rays, const rt_hit* hits, int64_t n, int32_t spp,
                             rt_obscurance* acc)
{
    const char* name = "rt_debug_obscurance_fold";
    const char* bad = n < 0 ? "n < 0" : spp <= 0 ? "spp <= 0" : nullptr;
    if (!bad && n == 0) return RT_OK;
    if (!bad && (!rays || !hits || !params || !acc)) bad = "null pointer";
    if (!bad && !obscurance_params_ok(params)) bad = kObscuranceParamsRule;
    if (bad) return bad_argument(name, bad);
    for (int64_t i = 0; i < n; i++) {
        rt_obscurance& a = acc[i];
        double sum[kObscuranceTerms] = {a.o, a.o2, a.bent[0], a.bent[1], a.bent[2]};
        for (int64_t at = i * spp; at < (i + 1) * spp; at++) {
            const rt_vec4d& d = rays[at].direction;
            obscurance_add(params->radius, params->power, d.x, d.y, d.z, hits[at].prim_id, hits[at].distance, sum, a.samples, a.hits);
        }
        a.o = sum[0];
        a.o2 = sum[1];
        a.bent[0] = sum[2];
        a.bent[1] = sum[3];
        a.bent[2] = sum[4];
    }
    return RT_OK;
}

int rt_obscurance_select_device(const rt_obscurance_select_params* P, const rt_obscurance* d_acc, int64_t n_records, uint32_t* d_list,
                                uint32_t cap, uint32_t* d_count, void* stream)
{
    const char* name = "rt_obscurance_select_device";
    int rc = check_select(name, P, d_acc, n_records, d_list, cap);
    if (rc != RT_OK) return rc;
    if (!d_count) return bad_argument(name, "null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SelectArgs A{*P, d_acc, (unsigned)n_records, (int)((n_records + 63) / 64)};
    SelectPass pass;
    rc = select_begin(name, (size_t)A.n_blocks, st, pass);
    if (rc != RT_OK) return rc;
    const unsigned grid = (unsigned)((A.n_blocks + 3) / 4);
    hipLaunchKernelGGL(obscurance_count_kernel, dim3(grid), dim3(256), 0, st, A, pass.S->masks, pass.S->counts);
    select_scan(pass, A.n_blocks, d_count, st);
    if (cap > 0)
        hipLaunchKernelGGL(obscurance_write_kernel, dim3(grid), dim3(256), 0, st, A.n_blocks, pass.S->masks, pass.S->counts, d_list, cap);
    return select_end(pass, st);
}

int64_t rt_debug_obscurance_select(const rt_obscurance_select_params* P, const rt_obscurance* acc, int64_t n_records, uint32_t* list,
                                   uint32_t cap)
{
    const int rc = check_select("rt_debug_obscurance_select", P, acc, n_records, list, cap);
    if (rc != RT_OK) return rc;
    int64_t n = 0;
    for (int64_t e = 0; e < n_records; e++) {
        if (!obscurance_active(*P, acc[e].o, acc[e].o2, acc[e].samples)) continue;
        if (n < (int64_t)cap) list[n] = (uint32_t)e;
        n++;
    }
    return n;
}

int rt_debug_obscurance_error(const rt_obscurance_select_params* P, const rt_obscurance* acc, int64_t n, double* se_out, double* mean_out)
{
    if (!P || n < 0 || (n > 0 && (!acc || !se_out || !mean_out)))
        return bad_argument("rt_debug_obscurance_error", "null pointer or n < 0");
    for (int64_t i = 0; i < n; i++) {
        se_out[i] = mean_out[i] = std::numeric_limits<double>::quiet_NaN();
        if (acc[i].samples < 2) continue;
        const double N = (double)acc[i].samples;
        obscurance_error(acc[i].o, acc[i].o2, N, se_out[i]);
        mean_out[i] = pg_div(acc[i].o, N);
    }
    return RT_OK;
}

} // extern "C"
