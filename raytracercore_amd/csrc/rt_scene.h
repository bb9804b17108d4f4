// rt_scene.h -- the scene object behind the C ABI and what the API's translation units share
// (rtcore_api.hip, scene_upload.hip, api_frame.hip, api_debug.hip, api_query.hip, api_select.hip, api_render_rays.hip,
// api_render_pixels.hip, api_render_probes.hip, api_shade_probes.hip, api_probe_depth.hip, api_probe_relocate.hip, api_obscurance.hip, chunk_pipeline.hip, api_adaptive.hip, api_denoise.hip, api_reproject.hip).
#pragma once
#include <algorithm>
#include <array>
#include <functional>
#include <string>
#include <vector>

#include "block_cull.h"
#include "host_scene.h"
#include "launch_params.h"
#include "rt_jit.h"
#include "rt_kernels.h"
#include "scene_records.h"

using namespace rtc;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                               \
            return e_ == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP;                                 \
        }                                                                                               \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t reserve(size_t count)
    {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void adopt(T* q, size_t count) // take ownership of a hipMalloc'd array
    {
        release();
        p = q;
        n = q ? count : 0;
    }
    hipError_t upload(const std::vector<T>& v)
    {
        hipError_t e = reserve(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// Pinned host staging (hipHostMalloc) for the host-buffer entry points: device -> host copies at
// DMA rate into it, then a multi-threaded pass into the caller's (pageable) arrays.
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t n = 0;
    ~HostBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t reserve(size_t count)
    {
        if (count <= n) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = count;
        return e;
    }
};

// The device arrays of one brute-force slot order (BruteOrder).
struct BruteDev {
    DevBuf<PrimF> prims;
    DevBuf<TestRec> tests;
    DevBuf<RectRec> rects;
    DevBuf<FrameRec> frames; // FrameRecs and BoxRecs
    DevBuf<GroupRec> groups;
    hipError_t upload(const BruteOrder& o)
    {
        hipError_t e = prims.upload(o.prims);
        if (e == hipSuccess) e = tests.upload(o.tests);
        if (e == hipSuccess) e = rects.upload(o.rects);
        if (e == hipSuccess) e = frames.upload(o.frames);
        if (e == hipSuccess) e = groups.upload(o.groups);
        return e;
    }
};

struct rt_scene {
    int device = 0;
    int n_cu = 256;
    rt_scene_params params{};
    std::vector<HostPrim> host;
    int traversal = RT_TRAVERSAL_AUTO, resolved = RT_TRAVERSAL_BRUTE;
    int variant = 0;
    int blocks_per_cu = 1;
    RefBvh ref;
    bool ref_built = false;
    SahBvh sah;   // host-built trees (empty when the GPU builder made them)
    Bvh4 bvh4;
    struct {
        int builder = RT_BVH_BUILDER_HOST; // the one that ran
        int n_nodes2 = 0, n_nodes4 = 0, root2 = 0, root4 = 0, depth2 = 0, stack4 = 0, rounds = 0;
        int leaves4 = 0, compact4 = 0; // leaf references of the wide tree, compact ones (kLeafCompact)
        float gpu_ms = 0.0f;
    } bvh;
    DevBuf<int32_t> order_d;      // GPU builder: primitive IDs in leaf order, planes appended
    // Outer records (host builder, large scenes): the axis-aligned rectangles left out of the tree
    // and tested as one brute-force group (world rects and closed boxes) when a query ends
    std::vector<char> bvh_outer;  // per primitive: 1 = outside the tree (empty: none)
    double ms_prepare = 0, ms_bvh = 0, ms_upload = 0;
    BruteLayout layout;           // the flat brute-force order's decomposition (build statistics)
    int group_max = 0;            // primitives per group of the grouped order
    DevScene dev{};
    // the flat and the grouped order; the BVH order: the tree's and the planes' prims and tests (built
    // by either builder, upload_scene) and the outer group's rects, BoxRecs (frames) and GroupRec
    BruteDev flat_d, grouped_d, bvh_d;
    DevBuf<float4> rows_bvh; // bvh_d.tests without the meta rows (compact leaves)
    std::vector<GroupRec> groups_gr_host; // in build order; uploaded nearest-first per camera
    // host copies of the brute-force records (the scene-specialised kernels, rt_jit.h)
    struct BruteHost {
        std::vector<GroupRec> groups; // the grouped order: in the current camera's upload order
        std::vector<RectRec> rects;
        std::vector<FrameRec> frames;
        std::vector<TestRec> tests;
    } flat_h, grouped_h;
    std::vector<XformF> xf_h;
    unsigned jit_gen = 0; // bumped by every camera change (and with it the grouped order's group order)
    struct {
        int variant = -1;          // the variant and group order the function was built for
        unsigned gen = 0;
        hipFunction_t fn = nullptr;
        int blocks_per_cu = 0;
        int status = 0;            // 1 built, 0 not used (off, or a BVH / staged-less variant), -1 failed
        double compile_ms = 0;
        bool from_cache = false;
        std::string error;
        std::string header;        // the generated scene header fn was built from
    } jit;
    double grouped_measured = 0; // calibrated brute-force cost ratio flat / grouped (AUTO picks grouped above 1.25)
    DevBuf<NodeF> nodes;
    DevBuf<Node4Q> nodes4;
    DevBuf<Node4Q> hot4;        // top of the wide tree, breadth-first, staged in LDS by the wide kernel
    DevBuf<XformF> xf;
    DevBuf<MatF> mats;
    DevBuf<float4> vnormals;
    DevBuf<PrimD> prims_d;
    DevBuf<XformD> xf_d;
    DevBuf<RefNode> ref_nodes;
    // work buffers
    DevBuf<unsigned int> counter;
    DevBuf<rt_key2> pkeys;       // pixel-key table of the brute-force kernels (PathParams::pkeys)
    bool pkeys_valid = false;
    uint64_t pkeys_seed = 0;
    DevBuf<float4> starts;       // start rows of the brute-force kernels (PathParams::starts), grown on demand
    DevBuf<int> stack_ovf;
    DevBuf<unsigned long long> rays;
    DevBuf<float4> partial;
    DevBuf<double> sum, colors;
    DevBuf<float> colors32;        // rt_render_tile_1spp: one pass as fp32 rgb in the caller's order
    HostBuf<unsigned char> stage;  // host-buffer entry points (rt_render_tile, rt_render_tile_1spp)
    HostBuf<unsigned long long> rays_h;
    static constexpr int kCopyChunks = 8; // chunked device -> host copies (copy_consume)
    std::array<hipEvent_t, kCopyChunks> copy_ev{};
    // rt_render_tile: band k's records are copied on copy_stream once band_ev[k] (recorded on the
    // scene's stream after the band's layout kernel) has fired, so band k + 1 renders meanwhile
    hipStream_t copy_stream = nullptr;
    std::array<hipEvent_t, kCopyChunks> band_ev{};
    DevBuf<uint32_t> samples, misses;
    DevBuf<int32_t> ids;
    // the chunked host entries' device slots (run_chunks, below, says which entry uses which) and the
    // events of the chunks' uploads
    DevBuf<rt_ray> query_rays;
    DevBuf<rt_hit> query_hits;
    DevBuf<double> occluded_t_max;
    DevBuf<unsigned char> occluded_out;
    DevBuf<uint32_t> occluded_counts;
    DevBuf<TileRec> render_rays_recs;
    DevBuf<uint32_t> pixel_list;
    DevBuf<PixelRec> pixel_recs;
    DevBuf<ProbeRec> probe_recs; // rt_render_probes: two chunks' accumulators, uploaded, folded into and downloaded
    std::array<hipEvent_t, 2> query_up_ev{};
    // rt_primary_hits_device: one chunk of camera rays, made and read on the caller's stream (its own
    // buffer: rt_query_rays fills query_rays from its copy stream)
    DevBuf<rt_ray> primary_rays;
    // rt_shade_probes_device: one chunk's eight segments per point, their ends and the any-hit answers, made
    // and read on the caller's stream; rt_shade_probes: the grid's L, one chunk of points and its results
    DevBuf<rt_ray> probe_seg_rays;
    DevBuf<double> probe_seg_t_max;
    DevBuf<unsigned char> probe_seg_occluded;
    DevBuf<double> shade_L, shade_out;
    // rt_render_probe_depth_device, rt_relocate_probes_device and rt_obscurance_surfels_device: one chunk's sample
    // rays and their closest hits, made and read on the caller's stream
    DevBuf<rt_ray> probe_depth_rays;
    DevBuf<rt_hit> probe_depth_hits;
    DevBuf<rt_surfel> shade_points; // (rt_relocate_probes_device: also a chunk's probe records)
    // run_items: the blocks per CU of each ItemSource's instance of `items_variant`
    int items_variant[ITEMS_SURFELS + 1] = {-1, -1, -1, -1, -1}, items_blocks_per_cu[ITEMS_SURFELS + 1] = {1, 1, 1, 1, 1};
    // the selection pass (api_select.hip): the caller's item list on the device, and the host-buffer
    // entry points' rays (one chunk) and results
    DevBuf<rt_select_item> select_items;
    DevBuf<rt_ray> select_rays;
    DevBuf<rt_selection> select_out;
    bool stats_on = false;      // launch the instrumented kernel (rt_scene_set_stats)
    float4* ray_log = nullptr;  // rt_debug_ray_log (instrumented BVH launches)
    unsigned int* ray_log_n = nullptr;
    unsigned int ray_log_cap = 0;
    int stats_blocks_per_cu = 1;
    DevBuf<unsigned long long> stats_buf;
    // rt_trace_paths: its launch is the instrumented kernel's, with the counters aimed at a scratch
    // block of its own (run_path), so stats_buf, an armed ray log and the scene-specialised kernel
    // stay as they are
    bool tracing = false;
    DevBuf<unsigned long long> trace_stats;
    DevBuf<float4> trace_rays, trace_samples, trace_out; // records and sample rows; both in the caller's order
    CameraD camd{};
    CameraF camf{};
    DevBuf<CameraF> camf_d;     // the path kernels read the camera from device memory (not kernel arguments)
    // ... and their launch parameters, from a ring of device slots filled from pinned host slots.
    // A slot is rewritten kParamRing launches later; its event (recorded after the slot's upload)
    // is waited on first, so a caller queueing more launches than that without a sync still
    // hands every launch its own parameters.
    static constexpr int kParamRing = 256;
    DevBuf<PathParams> params_d;
    PathParams* params_h = nullptr;
    std::array<hipEvent_t, kParamRing> slot_ev{};
    unsigned params_next = 0;
    // The block cull's records (PathParams::cull, plan_block_cull), cached by what they depend on: the
    // camera (cam_gen, bumped by rt_scene_set_camera), the window and the band set; the frame size
    // and the bound are the scene's.  A few entries, least recently used replaced, so that a host
    // which alternates among a few windows (rt_render_tile's column bands) builds each once.  An
    // entry is built in its pinned words and uploaded stream-ordered; `up` (recorded after the
    // upload) guards the pinned words against the next rebuild.
    struct CullEntry {
        bool valid = false;
        unsigned cam_gen = 0;
        CullWindow win{};
        int n_live = 0, n_blocks = 0;
        bool masks = false; // the record ends with the live blocks' unit masks (cull_masks_at, rt_kernels.h)
        uint64_t dead_px = 0, used = 0;
        DevBuf<unsigned int> dev;
        HostBuf<unsigned int> host;
        hipEvent_t up = nullptr;
    };
    // At least 3 entries, for launch overlap: a replaced entry's fresh record is uploaded on a launch set's
    // stream, which is behind both sets' path kernels and the set's own previous fold but not behind
    // the fold of the other set's latest launch, still queued on the caller's stream, which reads its
    // launch's record too.  The entry replaced is the least recently used, so with 3 or more entries it
    // is neither that launch's nor the one's before it; with 2 or fewer this would be a race.
    static constexpr int kCullEntries = 4;
    static_assert(kCullEntries >= 3, "launch overlap: a replaced cull entry must not be one of the last two launches'");
    std::array<CullEntry, kCullEntries> cull_cache;
    uint64_t cull_clock = 0;
    FlatUnits units;            // the flat order's test units and their boxes (scene_records.h), with the bound
    unsigned cam_gen = 0;
    bool has_camera = false;
    bool flat_overflow = false; // the flat brute-force order exceeds GroupRec's counts (BruteOrder::overflow)
    hipStream_t stream = nullptr;
    // Timing of the path kernels: the i-th launch records the event pair i % kTimeSlots, so a caller
    // can queue up to kTimeRing launches before it reads their durations (rt_kernel_times).  One pair
    // more than that is kept: the oldest entry's time is measured from its predecessor's end when the
    // two overlapped (launch overlap, below).
    static constexpr int kTimeRing = 64, kTimeSlots = kTimeRing + 1;
    std::array<hipEvent_t, kTimeSlots> t_start{}, t_end{};
    uint64_t launches = 0;
    // Launch overlap (run_path): rt_render_device and rt_render_bands_device alternate between two
    // launch sets, so that launch k + 1's path kernel, queued on its set's own stream, enters the SIMDs
    // that launch k's last waves leave.  A set is the work buffers a path kernel writes (partials,
    // dispensers, start rows, stack overflow area, a ray counter of its own in set_rays), the stream its
    // path kernel runs on and two events: path_done (after the path kernel, on the set's stream) and
    // fold_done (after the fold of its partials, on the caller's stream; the set's next launch waits for
    // it).  Set 0's buffers are the scene's (partial, counter, starts, stack_ovf above), which every other
    // operation uses, serially, once both sets are idle (done_ev below covers both folds); alt holds set 1's.
    struct LaunchSet {
        hipStream_t stream = nullptr;
        hipEvent_t path_done = nullptr, fold_done = nullptr;
        bool path_recorded = false, fold_recorded = false;
        bool after_serial = false; // a serial operation ran since the set's last launch: wait for done_ev
        bool after_shared = false; // the other set's stream rewrote shared state since: wait for shared_ev
    };
    std::array<LaunchSet, 2> sets;
    struct {
        DevBuf<unsigned int> counter;
        DevBuf<float4> starts, partial;
        DevBuf<int> stack_ovf;
    } alt;
    DevBuf<unsigned long long> set_rays; // one counter per set: the path kernel adds, the fold moves it to the caller's
    hipEvent_t shared_ev = nullptr;      // after a set's stream rewrote pixel keys or a cull record
    uint64_t overlapped = 0;             // overlapped launches so far (launch k of them uses set k & 1)
    int prev_w = 0, prev_h = 0, prev_spp = 0; // the previous launch of the two entries (launch_overlaps: repeats)
    int open_set = -1;                   // the set of the overlapped launch whose fold end_op closes, or -1
    // Launches share per-scene scratch (partials, work counter, stack overflow area).  The end of
    // the last render operation is recorded here; an operation on a different stream waits for it.
    hipEvent_t done_ev = nullptr;
    hipStream_t last_stream = nullptr;
    bool any_op = false;
    uint64_t device_bytes = 0;

    ~rt_scene()
    {
        if (jit.fn) jit_release(device, jit.fn); // (the stream is synchronised by rt_scene_destroy)
        if (params_h) (void)hipHostFree(params_h);
        for (hipEvent_t e : slot_ev)
            if (e) (void)hipEventDestroy(e);
        if (done_ev) (void)hipEventDestroy(done_ev);
        for (CullEntry& c : cull_cache)
            if (c.up) (void)hipEventDestroy(c.up);
        for (hipEvent_t e : copy_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : band_ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : query_up_ev)
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) {
            (void)hipStreamSynchronize(copy_stream);
            (void)hipStreamDestroy(copy_stream);
        }
        for (int i = 0; i < kTimeSlots; i++) {
            if (t_start[i]) (void)hipEventDestroy(t_start[i]);
            if (t_end[i]) (void)hipEventDestroy(t_end[i]);
        }
        for (LaunchSet& l : sets) { // (the streams are synchronised by rt_scene_destroy)
            if (l.path_done) (void)hipEventDestroy(l.path_done);
            if (l.fold_done) (void)hipEventDestroy(l.fold_done);
            if (l.stream) (void)hipStreamDestroy(l.stream);
        }
        if (shared_ev) (void)hipEventDestroy(shared_ev);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The host-buffer entry points' device -> host step.  queue_copy queues records [a, b) of d_src (after
// the work already on the scene's stream) into the same offsets of pinned staging, in k chunks whose
// arrivals are recorded by events; consume_copies then runs consume(stage, a, b) on the host pool
// for each chunk's items as soon as that chunk has landed, so the host pass over one chunk overlaps
// the DMA of the next (and whatever device work was queued after it).  Staging must be reserved
// for every queued record first.
struct CopyPlan {
    size_t a[rt_scene::kCopyChunks], b[rt_scene::kCopyChunks];
    int n = 0;
};

namespace rtc {

// scene_upload.hip
int builder_for(int n_bvh);  // the BVH builder (RT_BVH_BUILDER_HOST / _GPU) a scene of n_bvh non-plane primitives gets
int group_max_default();     // primitives per group of the grouped order, by the process's rt_set_jit state
int build_bvhs(rt_scene* s);
int upload_scene(rt_scene* s);
int ensure_ref_bvh(rt_scene* s);
int resolve_traversal(rt_scene* s);
int calibrate_grouping(rt_scene* s);
int prepare_jit(rt_scene* s);
int check_tile(rt_scene* s, int x0, int y0, int w, int h);
PathParams make_params(rt_scene* s, int x0, int y0, int w, int h, int spp, uint64_t seed, uint64_t base,
                       double chunk_npix = 0.0);
// may_overlap: the launch may run on a launch set's own stream (rt_scene::LaunchSet).  When it does,
// s->open_set names the set on return: the caller folds the partials on `stream` (run_path has made it
// wait for the path kernel), hands the fold set_rays.p + open_set to move into d_rays, and calls end_op.
int run_path(rt_scene* s, PathParams& p, unsigned long long* d_rays, hipStream_t stream, bool timed = true,
             bool may_overlap = false);
int upload_params(rt_scene* s, const PathParams& p, hipStream_t stream, const PathParams** d_out);
int end_op(rt_scene* s, hipStream_t stream);
int queue_copy(rt_scene* s, CopyPlan& plan, const void* d_src, size_t a, size_t b, size_t rec_bytes, int k,
               hipStream_t stream);
int consume_copies(rt_scene* s, const CopyPlan& plan, const std::function<void(const unsigned char*, size_t, size_t)>& consume);
// The scene's scratch (partials, work counter, stack overflow area) is shared: work on another stream than
// the last operation's waits for its end.
inline hipError_t wait_last_op(rt_scene* s, hipStream_t st)
{
    return s->any_op && st != s->last_stream ? hipStreamWaitEvent(st, s->done_ev, 0) : hipSuccess;
}
// chunk_pipeline.hip: the loop of every host entry that takes n of the caller's items (rt_query_rays,
// rt_occluded_rays, rt_occluded_surfels, rt_render_rays / _beams / _surfels, rt_render_probes, rt_render_list,
// rt_render_pixels), in chunks of C = min(largest, RTCORE_QUERY_CHUNK, cap, n) items, two of them resident;
// the order of its steps is argued at its definition.  An entry says what varies:
//   reserve(C, up, d_down)             its device buffers for two chunks of C items; it names the one the answers
//                                      come from, two slots of C x down_bytes, and keeps `up`, its part of the
//                                      pinned staging (2 C x up_bytes, 64-byte aligned, behind the two answer slots)
//   upload(k, first, m, slot)          chunk k, items [first, first + m) of the caller's: staged into slot's part of
//                                      `up` and queued from there to the device, all on copy_stream
//   launch(k, first, m, slot, st)      everything chunk k needs on the scene's stream, answers into slot
//   consume(stage, a, b, first, slot)  on the host pool: answer i in [a, b) of the staging is item first + (i - slot)
// slot = (k & 1) C is the chunk's offset, in items, in every two-chunk buffer.  The buffers are the scene's and
// shared by size, not by name: every entry's records travel in query_rays (a surfel is an rt_ray, a beam three)
// and its entry numbers in pixel_list; the segment ends of both occlusion entries in occluded_t_max; the answers
// in query_hits, occluded_out, occluded_counts, render_rays_recs (rays, beams, surfels), pixel_recs (pixels,
// lists) or probe_recs (probes: these also go up, with the sums the fold continues from).  An entry has consumed its last chunk when it returns, so the next call finds them free.
struct ChunkJob {
    int64_t n, largest, cap; // cap 0: none
    size_t down_bytes, up_bytes;
    bool one_piece;   // a chunk's answers come down as one copy (else in up to kCopyChunks pieces of at least 1 MB)
    bool count_rays;  // the render entries: s->rays zeroed before the first chunk and returned after the last
    std::function<int(size_t, unsigned char*, const void*&)> reserve;
    std::function<int(int64_t, size_t, size_t, size_t)> upload;
    std::function<int(int64_t, size_t, size_t, size_t, hipStream_t)> launch;
    std::function<void(const unsigned char*, size_t, size_t, size_t, size_t)> consume;
};
int run_chunks(rt_scene* s, const ChunkJob& job, uint64_t* rays_out = nullptr);
// The render entries' cap: a chunk's partials stay below 2^26 work items (1 GiB of 16-B partials), in whole
// blocks of 64 entries, whatever spp is; probe: the entry's launch record for 64 entries.  Below 64: spp is
// too large for one launch.
int64_t chunk_fit(const PathParams& probe);
// api_render_rays.hip: what rt_render_rays, rt_render_beams and rt_render_surfels share, a radiance query
// over a list of caller's records (rt_ray, rt_beam or rt_surfel) by the src instances of the path
// kernels.  rec_bytes: one record, a multiple of sizeof(rt_ray); chunk: most records of one chunk of the
// host entry; what: the records' name in messages; gather_mode: the surfels' rt_gather_mode (else 0).  render_list_device / render_list_host are the two entry points'
// bodies, with the name of the entry point for messages.
struct RenderList {
    ItemSource src;
    size_t rec_bytes;
    int64_t chunk;
    const char* what;
    int gather_mode = 0;
};
// The launch of an item-list instance of the path kernels (src: RAYS, BEAMS, SURFELS or PIXELS) and nothing
// after it: the caller has set the instance's own words of p (run_rays; pixel_list and a null cull) and
// folds p's partials.  what: the entry's items in messages ("rt_render_<what>: ...").
int run_items(rt_scene* s, ItemSource src, const char* what, PathParams& p, unsigned long long* d_count, hipStream_t stream);
// run_items for a list of records: kind's instance over the p.n_rays records at d_list; with d_index
// (rt_render_list, api_render_list.hip) item j is entry d_index[j] of n_records records, whose record lies
// at list position j (gathered) or at its entry number.
int run_rays(rt_scene* s, const RenderList& kind, PathParams& p, const void* d_list, unsigned long long* d_count,
             hipStream_t stream, const uint32_t* d_index, unsigned n_records, bool gathered);
// The argument and state checks of every entry over such a list (rt_render_probes' too, api_render_probes.hip),
// with the entry point's name for messages; RT_OK with *empty set for n == 0.
int check_render_rays(rt_scene* s, const void* rays, int64_t n, int32_t spp, const void* sum, const void* samples,
                      const void* misses, const char* name, bool* empty);
int render_list_device(rt_scene* s, const RenderList& kind, const char* name, const void* d_list, int64_t n, int32_t spp,
                       uint64_t seed, uint64_t sample_base, uint64_t stream_base, double* d_sum, uint32_t* d_samples,
                       uint32_t* d_misses, unsigned long long* d_count, void* stream);
int render_list_host(rt_scene* s, const RenderList& kind, const char* name, const void* list, int64_t n, int32_t spp,
                     uint64_t seed, uint64_t sample_base, uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples,
                     uint32_t* misses, uint64_t* rays_out);
// api_query.hip: what rt_query_rays, rt_occluded_rays and rt_occluded_surfels (api_occluded_surfels.hip) share.
constexpr int64_t kQueryChunk = 1 << 19;     // most items of one chunk of a host entry (run_chunks; beams: 2^18)
constexpr int64_t kQueryLaunchMax = 1 << 30; // rays of one launch (32-bit ray indices and dispenser)
// The generic kernel of the scene's traversal mode (path_variant's numbering).
int query_kernel(const rt_scene* s);
// The RT_QUERY_FAST launch record of n rays for that kernel (unstaged records) and its grid; the BVH
// kernel's ray dispenser is zeroed on `st` and its overflow area reserved.
int fill_query(rt_scene* s, int kernel, int blocks_per_cu, const rt_ray* d_rays, unsigned n, hipStream_t st, QueryParams& p,
               int& grid);
// rt_occluded_rays' launch over n <= kQueryLaunchMax segments on `st` (d_t_max null: rays), after the stream
// ordering is settled; rt_shade_probes_device (api_shade_probes.hip) runs it over the segments it makes.
int launch_segments(rt_scene* s, int32_t mode, const rt_ray* d_rays, const double* d_t_max, unsigned n, unsigned char* d_out,
                    hipStream_t st);
// rt_query_rays' launch over n <= kQueryLaunchMax rays on `st`, after the stream ordering is settled;
// rt_render_probe_depth_device (api_probe_depth.hip) and rt_obscurance_surfels_device (api_obscurance.hip) run it
// over the sample rays they make.
int launch_rays(rt_scene* s, int32_t mode, const rt_ray* d_rays, unsigned n, rt_hit* d_hits, hipStream_t st);
// api_render_surfels.hip: rt_debug_surfel_rays_device's launch for total = n x spp samples on `st`.
int launch_surfel_rays(int32_t mode, const rt_surfel* d_surfels, unsigned long long total, unsigned spp, uint64_t seed,
                       uint64_t sample_base, uint64_t stream_base, rt_ray* d_rays_out, hipStream_t st);
// api_render_pixels.hip: rt_render_pixels' list check (every entry below npix, none twice); null, or
// what is wrong with entry *at
const char* check_pixel_list(const uint32_t* pixels, int64_t n, uint64_t npix, int64_t* at);
int copy_consume(rt_scene* s, const void* d_src, size_t n_items, size_t rec_bytes,
                 const std::function<void(const unsigned char*, size_t, size_t)>& consume);

} // namespace rtc
