// api_frame.hip -- the C ABI's row-band renders and the multi-GPU frame pipeline (rt_frame).
#include <rccl/rccl.h>

#include <cstring>
#include <memory>
#include <thread>

#include "rt_scene.h"

// ------------------------------------------------------------------ row bands (multi-GPU) ----
// A band set (band, stride, offset) is frame rows {y : (y / band) % stride == offset}: device g of
// n owns set (8, n, g), interleaved for load balance (die.txt's background rows cost one ray per
// sample).  On the device a set is rendered as a tile of band_set_rows() rows, tile row r being
// frame row ((r / band) * stride + offset) * band + r % band (PathParams::band), into planar
// accumulators whose planes are `plane` elements apart -- the slot of rt_frame's gather, sized for
// the tallest set, so a shorter set leaves the end of each plane unused.
struct rt_frame {
    int n = 0, W = 0, H = 0, band = 8; // 8-row bands: any split of 1080 or 2160 rows is within one band of even
    std::vector<int> rows;            // rows of device g's band set
    size_t slot_pix = 0, slot_bytes = 0;
    std::vector<rt_scene*> scenes;
    std::vector<ncclComm_t> comms; // one rank per device (n = 1 too: one code path, a local copy)
    // Two pipeline stages (rt_frame_submit / rt_frame_collect): stage j holds every device's gather
    // slot, device 0's receive buffer (n slots), the pinned host copy of the gathered slots and of
    // the devices' ray counts, and the event that says the host copy has landed.
    static constexpr int kStages = 2;
    struct Stage {
        std::vector<unsigned char*> sendb; // per device: Σr | Σg | Σb fp64, samples, misses u32
        unsigned char* recvb = nullptr;    // device 0
        unsigned char* host = nullptr;     // pinned: n slots, then n ray counts
        hipEvent_t gathered = nullptr;     // device 0's render stream: the gather is complete
        hipEvent_t landed = nullptr;       // device 0's copy stream: the host copy is complete
        std::vector<hipEvent_t> rays_ev;   // per device: its ray count has been copied
    } st[kStages];
    hipStream_t copy_stream = nullptr;     // device 0: host copies, off the render streams
    unsigned long long submitted = 0, collected = 0; // renders queued / merged (at most kStages apart)
    int inject = 0;                        // rt_frame_inject_fault (tests)

    unsigned long long* host_rays(int j) { return reinterpret_cast<unsigned long long*>(st[j].host + slot_bytes * n); }
    ~rt_frame()
    {
        for (ncclComm_t c : comms) (void)ncclCommDestroy(c);
        for (auto& S : st) {
            for (int g = 0; g < (int)S.sendb.size(); g++)
                if (S.sendb[g]) {
                    (void)hipSetDevice(scenes[g]->device);
                    (void)hipFree(S.sendb[g]);
                }
            for (int g = 0; g < (int)S.rays_ev.size(); g++)
                if (S.rays_ev[g]) {
                    (void)hipSetDevice(scenes[g]->device);
                    (void)hipEventDestroy(S.rays_ev[g]);
                }
            if (!scenes.empty() && scenes[0]) (void)hipSetDevice(scenes[0]->device);
            if (S.recvb) (void)hipFree(S.recvb);
            if (S.landed) (void)hipEventDestroy(S.landed);
            if (S.gathered) (void)hipEventDestroy(S.gathered);
            if (S.host) (void)hipHostFree(S.host);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (rt_scene* s : scenes)
            if (s) rt_scene_destroy(s);
    }
};

namespace {

// Queues one band set's render on stream: path kernel + accumulate into d_slot (added to).
int render_band_set(rt_scene* s, int band, int stride, int offset, int rows, size_t plane, int spp, uint64_t seed,
                    uint64_t sample_base, unsigned char* d_slot, unsigned long long* d_rays, hipStream_t stream)
{
    double* d_sum = reinterpret_cast<double*>(d_slot);
    uint32_t* d_n = reinterpret_cast<uint32_t*>(d_sum + 3 * plane);
    uint32_t* d_m = d_n + plane;
    PathParams p = make_params(s, 0, 0, s->params.width, rows, spp, seed, sample_base);
    set_band(p, band, stride, offset);
    int rc = run_path(s, p, d_rays, stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate(p, d_sum, d_n, d_m, stream, plane));
    return end_op(s, stream);
}

} // namespace

extern "C" {

int rt_render_bands(rt_scene* s, int32_t band, int32_t band_stride, int32_t band_offset, int32_t spp, uint64_t seed,
                    uint64_t sample_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    if (!s || band <= 0 || band_stride <= 0 || band_offset < 0 || band_offset >= band_stride || spp < 0 || !sum_rgb ||
        !samples || !misses) {
        set_error("rt_render_bands: bad argument");
        return RT_ERR_ARG;
    }
    if (!s->has_camera) {
        set_error("no camera set (rt_scene_set_camera)");
        return RT_ERR_STATE;
    }
    const int W = s->params.width, H = s->params.height;
    const int rows = band_set_rows(H, band, band_stride, band_offset);
    if (rows == 0 || spp == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const size_t plane = (size_t)band_slot_rows(H, band, band_stride) * W; // rt_frame's slot layout
    const size_t bytes = plane * (3 * sizeof(double) + 2 * sizeof(uint32_t));
    DevBuf<unsigned char> slot;
    HIP_TRY(slot.reserve(bytes));
    HIP_TRY(hipMemsetAsync(slot.p, 0, bytes, s->stream));
    HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
    int rc = render_band_set(s, band, band_stride, band_offset, rows, plane, spp, seed, sample_base, slot.p, s->rays.p,
                             s->stream);
    if (rc != RT_OK) return rc;
    std::vector<unsigned char> host(bytes);
    unsigned long long hr = 0;
    HIP_TRY(hipMemcpyAsync(host.data(), slot.p, bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(&hr, s->rays.p, sizeof hr, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    scatter_band_set(host.data(), plane, W, H, band, band_stride, band_offset, sum_rgb, samples, misses);
    if (rays_out) *rays_out += hr;
    return RT_OK;
}

int rt_render_bands_device(rt_scene* s, int32_t band, int32_t band_stride, int32_t band_offset, int32_t spp,
                           uint64_t seed, uint64_t sample_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                           uint64_t plane, unsigned long long* d_rays, void* stream)
{
    if (!s || band <= 0 || band_stride <= 0 || band_offset < 0 || band_offset >= band_stride || spp <= 0 || !d_sum ||
        !d_samples || !d_misses || !d_rays) {
        set_error("rt_render_bands_device: bad argument");
        return RT_ERR_ARG;
    }
    if (!s->has_camera) {
        set_error("no camera set (rt_scene_set_camera)");
        return RT_ERR_STATE;
    }
    const int W = s->params.width, H = s->params.height;
    const int rows = band_set_rows(H, band, band_stride, band_offset);
    if (plane == 0) plane = (uint64_t)band_slot_rows(H, band, band_stride) * W;
    if (plane < (uint64_t)rows * W) {
        set_error("rt_render_bands_device: plane stride smaller than the band set");
        return RT_ERR_ARG;
    }
    if (rows == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    // the slot's sample/miss planes follow the sum planes only in rt_frame; here they are separate
    // buffers, each row-major over the set with the same plane stride as the sums
    double* sum = d_sum;
    uint32_t* n = d_samples;
    uint32_t* m = d_misses;
    PathParams p = make_params(s, 0, 0, W, rows, spp, seed, sample_base);
    set_band(p, band, band_stride, band_offset);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_path(s, p, d_rays, st, true, true);
    if (rc != RT_OK) return rc;
    HIP_TRY(launch_accumulate(p, sum, n, m, st, (size_t)plane, s->open_set >= 0 ? s->set_rays.p + s->open_set : nullptr,
                              d_rays));
    return end_op(s, st);
}

int rt_band_rows(int32_t height, int32_t band, int32_t band_stride, int32_t band_offset)
{
    if (height < 0 || band <= 0 || band_stride <= 0 || band_offset < 0 || band_offset >= band_stride) {
        set_error("rt_band_rows: bad argument");
        return RT_ERR_ARG;
    }
    return band_set_rows(height, band, band_stride, band_offset);
}

int rt_band_slot_rows(int32_t height, int32_t band, int32_t band_stride)
{
    if (height < 0 || band <= 0 || band_stride <= 0) {
        set_error("rt_band_slot_rows: bad argument");
        return RT_ERR_ARG;
    }
    return band_slot_rows(height, band, band_stride);
}

int rt_scatter_band_slot(const void* slot, uint64_t plane, int32_t width, int32_t height, int32_t band,
                         int32_t band_stride, int32_t band_offset, rt_color* sum_rgb, uint32_t* samples,
                         uint32_t* misses)
{
    if (!slot || !sum_rgb || !samples || !misses || width <= 0 || height <= 0 || band <= 0 || band_stride <= 0 ||
        band_offset < 0 || band_offset >= band_stride ||
        plane < (uint64_t)band_set_rows(height, band, band_stride, band_offset) * (uint64_t)width) {
        set_error("rt_scatter_band_slot: bad argument");
        return RT_ERR_ARG;
    }
    scatter_band_set(static_cast<const unsigned char*>(slot), (size_t)plane, width, height, band, band_stride,
                     band_offset, sum_rgb, samples, misses);
    return RT_OK;
}

int rt_frame_create(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims, const rt_camera* camera,
                    int32_t n_gpus, rt_frame** out)
{
    if (!params || !camera || !out || n_gpus <= 0 || params->width <= 0 || params->height <= 0) {
        set_error("rt_frame_create: bad argument");
        return RT_ERR_ARG;
    }
    *out = nullptr;
    if (n_gpus > rt_device_count()) {
        set_error("rt_frame_create: not enough devices");
        return RT_ERR_NODEVICE;
    }
    std::unique_ptr<rt_frame> f(new rt_frame);
    f->n = n_gpus;
    f->W = params->width;
    f->H = params->height;
    for (int g = 0; g < n_gpus; g++) f->rows.push_back(band_set_rows(f->H, f->band, n_gpus, g));
    f->slot_pix = (size_t)band_slot_rows(f->H, f->band, n_gpus) * f->W;
    f->slot_bytes = f->slot_pix * (3 * sizeof(double) + 2 * sizeof(uint32_t));
    f->scenes.assign(n_gpus, nullptr);
    for (auto& S : f->st) {
        S.sendb.assign(n_gpus, nullptr);
        S.rays_ev.assign(n_gpus, nullptr);
    }
    std::vector<int> devs(n_gpus);
    for (int g = 0; g < n_gpus; g++) {
        devs[g] = g;
        int rc = rt_scene_create(params, prims, n_prims, g, &f->scenes[g]);
        if (rc == RT_OK) rc = rt_scene_set_camera(f->scenes[g], camera);
        if (rc != RT_OK) return rc;
        HIP_TRY(hipSetDevice(g));
        for (auto& S : f->st) {
            HIP_TRY(hipMalloc(&S.sendb[g], f->slot_bytes));
            HIP_TRY(hipEventCreateWithFlags(&S.rays_ev[g], hipEventDisableTiming));
        }
    }
    HIP_TRY(hipSetDevice(0));
    HIP_TRY(hipStreamCreateWithFlags(&f->copy_stream, hipStreamNonBlocking));
    for (auto& S : f->st) {
        HIP_TRY(hipMalloc(&S.recvb, f->slot_bytes * n_gpus));
        HIP_TRY(hipHostMalloc(&S.host, f->slot_bytes * n_gpus + sizeof(unsigned long long) * n_gpus,
                              hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&S.landed, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&S.gathered, hipEventDisableTiming));
    }
    f->comms.assign(n_gpus, nullptr);
    if (ncclCommInitAll(f->comms.data(), n_gpus, devs.data()) != ncclSuccess) {
        f->comms.clear();
        set_error("rt_frame_create: ncclCommInitAll failed");
        return RT_ERR_NCCL;
    }
    *out = f.release();
    return RT_OK;
}

int rt_frame_set_camera(rt_frame* f, const rt_camera* camera)
{
    if (!f || !camera) {
        set_error("rt_frame_set_camera: bad argument");
        return RT_ERR_ARG;
    }
    for (rt_scene* s : f->scenes) {
        int rc = rt_scene_set_camera(s, camera);
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

namespace {

// Drops every queued stage after a failure: waits for the devices' streams, so that no queued
// copy still writes a stage's buffers, and restarts the pipeline empty.
void frame_drain(rt_frame* f)
{
    for (rt_scene* s : f->scenes) {
        (void)hipSetDevice(s->device);
        (void)hipStreamSynchronize(s->stream);
    }
    (void)hipSetDevice(f->scenes[0]->device);
    (void)hipStreamSynchronize(f->copy_stream);
    f->submitted = f->collected = 0;
}

// The gather of stage j: every device's slot onto device 0, one grouped RCCL call.  The group is
// closed on every path (an open group would swallow the next call's gathers).
int frame_gather(rt_frame* f, int j)
{
    if (ncclGroupStart() != ncclSuccess) {
        set_error("rt_frame_render: ncclGroupStart failed");
        return RT_ERR_NCCL;
    }
    int rc = RT_OK;
    for (int g = 0; g < f->n && rc == RT_OK; g++) {
        if (f->inject == 1) { // rt_frame_inject_fault: a failure inside the group, before any gather
            f->inject = 0;
            set_error("rt_frame_render: injected fault inside the gather group");
            rc = RT_ERR_HIP;
            break;
        }
        const hipError_t e = hipSetDevice(f->scenes[g]->device);
        if (e != hipSuccess) {
            set_error(std::string("rt_frame_render: ") + hipGetErrorString(e));
            rc = RT_ERR_HIP;
            break;
        }
        if (ncclGather(f->st[j].sendb[g], g == 0 ? f->st[j].recvb : nullptr, f->slot_bytes, ncclUint8, 0, f->comms[g],
                       f->scenes[g]->stream) != ncclSuccess) {
            set_error("rt_frame_render: ncclGather failed");
            rc = RT_ERR_NCCL;
        }
    }
    if (ncclGroupEnd() != ncclSuccess && rc == RT_OK) {
        set_error("rt_frame_render: ncclGather failed");
        rc = RT_ERR_NCCL;
    }
    return rc;
}

int frame_submit(rt_frame* f, int32_t spp, uint64_t seed, uint64_t sample_base)
{
    const int j = (int)(f->submitted % rt_frame::kStages);
    auto& S = f->st[j];
    rt_scene* s0 = f->scenes[0];
    // every device renders its band set into its slot of stage j, concurrently (asynchronous launches);
    // the stage's previous host copy has been collected (at most kStages in flight), so its buffers
    // are free once device 0's copy stream has passed it, which the render streams wait for
    for (int g = 0; g < f->n; g++) {
        rt_scene* s = f->scenes[g];
        HIP_TRY(hipSetDevice(s->device));
        if (g == 0) HIP_TRY(hipStreamWaitEvent(s->stream, S.landed, 0));
        HIP_TRY(hipMemsetAsync(S.sendb[g], 0, f->slot_bytes, s->stream));
        HIP_TRY(hipMemsetAsync(s->rays.p, 0, sizeof(unsigned long long), s->stream));
        if (f->rows[g] > 0) {
            int rc = render_band_set(s, f->band, f->n, g, f->rows[g], f->slot_pix, spp, seed, sample_base, S.sendb[g],
                                     s->rays.p, s->stream);
            if (rc != RT_OK) return rc;
        }
        // the ray count, before the next stage's render zeroes it (pinned: the copy is asynchronous)
        HIP_TRY(hipMemcpyAsync(f->host_rays(j) + g, s->rays.p, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               s->stream));
        HIP_TRY(hipEventRecord(S.rays_ev[g], s->stream));
    }
    // the slots meet on device 0 through one RCCL gather over xGMI
    int rc = frame_gather(f, j);
    if (rc != RT_OK) return rc;
    // the host copy on device 0's copy stream, so that the next stage's render does not queue behind it
    HIP_TRY(hipSetDevice(s0->device));
    HIP_TRY(hipEventRecord(S.gathered, s0->stream));
    HIP_TRY(hipStreamWaitEvent(f->copy_stream, S.gathered, 0));
    HIP_TRY(hipMemcpyAsync(S.host, S.recvb, f->slot_bytes * f->n, hipMemcpyDeviceToHost, f->copy_stream));
    HIP_TRY(hipEventRecord(S.landed, f->copy_stream));
    f->submitted++;
    return RT_OK;
}

int frame_collect(rt_frame* f, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    const int j = (int)(f->collected % rt_frame::kStages);
    auto& S = f->st[j];
    HIP_TRY(hipSetDevice(f->scenes[0]->device));
    HIP_TRY(hipEventSynchronize(S.landed));
    for (int g = 0; g < f->n; g++) {
        HIP_TRY(hipSetDevice(f->scenes[g]->device));
        HIP_TRY(hipEventSynchronize(S.rays_ev[g]));
    }
    for (int g = 0; g < f->n; g++)
        scatter_band_set(S.host + f->slot_bytes * g, f->slot_pix, f->W, f->H, f->band, f->n, g, sum_rgb, samples,
                         misses);
    if (rays_out)
        for (int g = 0; g < f->n; g++) *rays_out += f->host_rays(j)[g];
    f->collected++;
    return RT_OK;
}

} // namespace

int rt_frame_submit(rt_frame* f, int32_t spp, uint64_t seed, uint64_t sample_base)
{
    if (!f || spp <= 0) {
        set_error("rt_frame_submit: bad argument");
        return RT_ERR_ARG;
    }
    if (f->submitted - f->collected >= (unsigned long long)rt_frame::kStages) {
        set_error("rt_frame_submit: two renders in flight; rt_frame_collect the oldest first");
        return RT_ERR_STATE;
    }
    const int rc = frame_submit(f, spp, seed, sample_base);
    if (rc != RT_OK) frame_drain(f);
    return rc;
}

int rt_frame_collect(rt_frame* f, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    if (!f || !sum_rgb || !samples || !misses) {
        set_error("rt_frame_collect: bad argument");
        return RT_ERR_ARG;
    }
    if (f->collected == f->submitted) {
        set_error("rt_frame_collect: nothing submitted");
        return RT_ERR_STATE;
    }
    const int rc = frame_collect(f, sum_rgb, samples, misses, rays_out);
    if (rc != RT_OK) frame_drain(f);
    return rc;
}

int rt_frame_render(rt_frame* f, int32_t spp, uint64_t seed, uint64_t sample_base, rt_color* sum_rgb,
                    uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    if (!f || spp < 0 || !sum_rgb || !samples || !misses) {
        set_error("rt_frame_render: bad argument");
        return RT_ERR_ARG;
    }
    if (spp == 0) return RT_OK;
    if (f->submitted != f->collected) {
        set_error("rt_frame_render: renders submitted and not collected");
        return RT_ERR_STATE;
    }
    int rc = rt_frame_submit(f, spp, seed, sample_base);
    if (rc == RT_OK) rc = rt_frame_collect(f, sum_rgb, samples, misses, rays_out);
    return rc;
}

int rt_frame_inject_fault(rt_frame* f, int32_t point)
{
    if (!f || point < 0 || point > 1) {
        set_error("rt_frame_inject_fault: bad argument");
        return RT_ERR_ARG;
    }
    f->inject = point;
    return RT_OK;
}

void rt_frame_destroy(rt_frame* f)
{
    if (!f) return;
    for (rt_scene* s : f->scenes)
        if (s) {
            (void)hipSetDevice(s->device);
            (void)hipStreamSynchronize(s->stream);
        }
    if (f->copy_stream) {
        (void)hipSetDevice(f->scenes[0]->device);
        (void)hipStreamSynchronize(f->copy_stream);
    }
    delete f;
}

int rt_render_frame_multi(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims,
                          const rt_camera* camera, int32_t n_gpus, int32_t spp, uint64_t seed, uint64_t sample_base,
                          rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out)
{
    if (!sum_rgb || !samples || !misses || spp < 0) {
        set_error("rt_render_frame_multi: bad argument");
        return RT_ERR_ARG;
    }
    rt_frame* f = nullptr;
    int rc = rt_frame_create(params, prims, n_prims, camera, n_gpus, &f);
    if (rc == RT_OK) rc = rt_frame_render(f, spp, seed, sample_base, sum_rgb, samples, misses, rays_out);
    rt_frame_destroy(f);
    return rc;
}

} // extern "C"
