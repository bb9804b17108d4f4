// chunk_pipeline.hip -- the double-buffered loop of the host entries that take the caller's items in
// chunks (ChunkJob, rt_scene.h): upload k + 1 and download k - 1 beside kernel k.
#include <cstdlib>

#include "rt_scene.h"

namespace rtc {

constexpr uint64_t kChunkItems = 1ull << 26; // most work items of one chunk: 1 GiB of 16-B partials

int64_t chunk_fit(const PathParams& probe) { return (int64_t)(kChunkItems / ((uint64_t)probe.n_chunks * 64u)) * 64; }

// Chunk k's items go through pinned staging to device slot k & 1 on copy_stream (job.upload), its kernels
// run on the scene's stream once they have landed (job.launch), and its answers come back on copy_stream
// (queue_copy) into the staging slot the host pool then reads (consume_copies, job.consume).  The copy
// stream's order is upload k + 1, download k: so chunk k's kernels run beside download k - 1 and upload
// k + 1, and a slot (device or pinned) is rewritten only after what last read it: upload k + 1 follows
// download k - 1, which followed kernel k - 1, and the host refills a pinned item slot after it has
// consumed the download queued behind that slot's previous upload.
// The two chunks' CopyPlans share the scene's one set of copy_ev: queue_copy records copy_ev[0 ..]
// whichever plan it fills.  So consume(k - 1), which waits on them piece by piece, comes before
// queue_copy(k), which records them anew: after it they would stand for chunk k's pieces, and the host
// would sit out kernel k and download k before it read a record of chunk k - 1, the overlap lost.
// consume(k - 1) also precedes upload(k + 1) and, an iteration later, queue_copy(k + 1), which rewrite
// the pinned slots chunk k - 1 used.
// The ray counter is one word that every chunk's kernel adds to; its copy to rays_h is queued on
// copy_stream behind the last kernel (band_ev) and ahead of the last chunk's answers, so it has landed
// when the last consume, which waits for those, returns.
int run_chunks(rt_scene* s, const ChunkJob& job, uint64_t* rays_out)
{
    int64_t chunk = job.largest;
    if (const char* e = getenv("RTCORE_QUERY_CHUNK")) chunk = std::max<int64_t>(1, std::min<int64_t>(job.largest, atoll(e)));
    if (job.cap) chunk = std::min(chunk, job.cap);
    chunk = std::min(chunk, job.n);
    HIP_TRY(hipSetDevice(s->device));
    if (!s->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamSynchronize(s->copy_stream)); // (copies a failed call left behind: see rt_render_tile)
    const size_t C = (size_t)chunk;
    // pinned staging: the two answer slots (at the offsets queue_copy gives them), then the entry's uploads
    const size_t up_at = (2 * C * job.down_bytes + 63) & ~(size_t)63;
    HIP_TRY(s->stage.reserve(up_at + 2 * C * job.up_bytes));
    const void* d_down = nullptr;
    int rc = job.reserve(C, s->stage.p + up_at, d_down);
    if (rc != RT_OK) return rc;
    if (job.count_rays) HIP_TRY(s->rays_h.reserve(1));
    for (int j = 0; j < 2; j++) {
        if (!s->query_up_ev[j]) HIP_TRY(hipEventCreateWithFlags(&s->query_up_ev[j], hipEventDisableTiming));
        if (!s->band_ev[j]) HIP_TRY(hipEventCreateWithFlags(&s->band_ev[j], hipEventDisableTiming));
    }
    hipStream_t st = s->stream;
    HIP_TRY(wait_last_op(s, st));
    if (job.count_rays) HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), st));
    const int64_t K = (job.n + chunk - 1) / chunk;
    auto first = [&](int64_t k) { return (size_t)(k * chunk); };
    auto count = [&](int64_t k) { return (size_t)std::min(chunk, job.n - k * chunk); };
    auto slot = [&](int64_t k) { return (size_t)(k & 1) * C; };
    auto upload = [&](int64_t k) -> int {
        const int urc = job.upload(k, first(k), count(k), slot(k));
        if (urc != RT_OK) return urc;
        HIP_TRY(hipEventRecord(s->query_up_ev[k & 1], s->copy_stream));
        return RT_OK;
    };
    CopyPlan plans[2];
    auto consume = [&](int64_t k) -> int {
        const size_t f = first(k), sl = slot(k);
        return consume_copies(s, plans[k & 1],
                              [&](const unsigned char* stage, size_t a, size_t b) { job.consume(stage, a, b, f, sl); });
    };
    rc = upload(0);
    if (rc != RT_OK) return rc;
    for (int64_t k = 0; k < K; k++) {
        const size_t m = count(k);
        HIP_TRY(hipStreamWaitEvent(st, s->query_up_ev[k & 1], 0));
        rc = job.launch(k, first(k), m, slot(k), st);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipEventRecord(s->band_ev[k & 1], st));
        if (k >= 1) {
            rc = consume(k - 1);
            if (rc != RT_OK) return rc;
        }
        if (k + 1 < K) {
            rc = upload(k + 1);
            if (rc != RT_OK) return rc;
        }
        HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->band_ev[k & 1], 0));
        if (job.count_rays && k + 1 == K)
            HIP_TRY(hipMemcpyAsync(s->rays_h.p, s->rays.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->copy_stream));
        plans[k & 1] = CopyPlan{};
        const size_t pieces =
            job.one_piece ? 1 : std::max<size_t>(1, std::min<size_t>(rt_scene::kCopyChunks, (m * job.down_bytes) >> 20));
        rc = queue_copy(s, plans[k & 1], d_down, slot(k), slot(k) + m, job.down_bytes, (int)pieces, s->copy_stream);
        if (rc != RT_OK) return rc;
    }
    rc = end_op(s, st);
    if (rc != RT_OK) return rc;
    rc = consume(K - 1);
    if (rc != RT_OK) return rc;
    if (job.count_rays && rays_out) *rays_out += s->rays_h.p[0];
    return RT_OK;
}

} // namespace rtc
