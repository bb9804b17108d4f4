// launch_params.h -- host-side planning of a path-tracing launch (launch_params.cpp): the work
// decomposition of a tile (PathParams), the order its items are dealt in, and the row bands of the
// multi-GPU frame.  No HIP calls.
#pragma once
#include "rt_kernels.h"

namespace rtc {

// kernel: 0 flat, 1 grouped brute force, 2 / 3 the BVH kernels; chunks_over / pool_over > 0 (the host
// check, rt_debug_item_order): chunks per pixel and items per ticket instead of the tuned ones.
PathParams make_params_for(int kernel, int chunks_over, int pool_over, int x0, int y0, int w, int h, int spp,
                           uint64_t seed, uint64_t base, double chunk_npix);
// rt_render_rays: the launch record of n caller-supplied rays (a tile 8 wide, so that ray i is pixel
// i & 63 of block i >> 6; p.ray_list is set by the caller), and the most rays one launch takes at
// this spp (32-bit item indices).
PathParams make_params_rays(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, uint64_t stream_base);
int64_t render_rays_max_n(int kernel, int spp);
// rt_render_pixels: the launch record of a list of n frame pixels of a width x height frame, planned as
// make_params_rays plans n rays (p.pixel_list is set by the caller); render_rays_max_n bounds n.
PathParams make_params_pixels(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, int width, int height);
// rt_render_probes: the launch record of n probes, planned as make_params_rays plans n rays but with spp
// chunks per probe: one sample per work item whatever spp is (chunk = 1, n_chunks = spp rounded up to a
// power of two), so that the partial row of item (probe i, chunk k) is sample k's colour and count.
// probes_max_n bounds n: the most probes, in whole blocks of 64, whose n_chunks slots stay within 2^26 work
// items (1 GiB of partials); 0 when not even 64 fit (spp > 2^20).  Call it first: it takes any spp > 0.
PathParams make_params_probes(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, uint64_t stream_base);
int64_t probes_max_n(int spp);
// The order in which the dispensers deal p's work items, from p's chunks, pool and ranges.
void set_item_order(PathParams& p);
// Plans p's item ranges and tickets (set_item_order) over n_blocks blocks; p.n_pad = 64 n_blocks.
void set_blocks(PathParams& p, int n_blocks);
// Band-set launch: tile row r is frame row ((r / band) * stride + offset) * band + r % band.
void set_band(PathParams& p, int band, int stride, int offset);
// Every ticket of p's dispensers through ticket_items, as (range, first item, items) triples into
// out while they fit in cap_words; returns the number of tickets.
int64_t list_tickets(const PathParams& p, uint32_t* out, int64_t cap_words);

// Start rows (PathParams::starts, refill in kernels_path.hip): whether a tile launch of `kernel` with
// `chunk` samples per item on a grid of grid_blocks blocks of 256 gets them, and the buffer they take.
// instrumented / vertex_normals: the launch runs an instance without them.  camera_kind / dof: the
// camera's kind (rt_camera_kind) and whether it has depth of field.
constexpr int kStartRowsMaxChunk = 16;          // rows per wave: an item's samples
constexpr size_t kStartRowsCap = 256u << 20;    // bytes of the buffer (a 1080p frame at 256 spp: 79 MB)
struct StartRowsPlan {
    bool on;
    int rows;      // per wave (= chunk), 0 when off
    size_t bytes;  // grid_blocks * 4 waves * rows * 64 lanes * 16 B, 0 when off
};
StartRowsPlan plan_start_rows(int kernel, bool instrumented, bool vertex_normals, int camera_kind, bool dof, int chunk,
                              int grid_blocks);

// Launch overlap (run_path, scene_upload.hip; rt_scene::LaunchSet).  launch_overlaps: whether a launch runs
// on a launch set's own stream beside the previous launch's tail: only the device entries that repeat in
// a progressive render (rt_render_device, rt_render_bands_device) and only a launch that repeats the
// width, height and samples of the one before it through those entries (a progressive render does; a
// small launch beside a large one would wait for the slots the large one's persistent waves hold, end
// after its successor, and rt_kernel_times could no longer say which time was whose), only the brute-force kernels
// (the BVH kernel is bound by the vector-memory pipeline, and a second kernel's waves beside its last ones cost
// the 1M-triangle launch more than the tail gives: 38.75-38.79 -> 39.32-39.46 ms per step), never an
// instrumented or tracing launch, not when the second set's partials would exceed kOverlapSetCap bytes,
// and not under RTCORE_LAUNCH_OVERLAP=0 (read per launch).
constexpr size_t kOverlapSetCap = 4ull << 30; // (the 1M-triangle 1080p x 64 spp launch: 2.1 GB)
bool launch_overlaps(bool device_entry, bool repeats, bool bvh, bool instrumented, bool tracing, size_t partial_bytes);
// overlap_wait: what an overlapped launch waits for before it touches state that the other set's path
// kernel, possibly in flight, reads: nothing when the launch rewrites none of it; the other set's
// path_done on its stream when it rebuilds the pixel keys (a new seed) or uploads a fresh cull record;
// the same on the host when memory is freed: a cull entry replaced, a scene-specialised kernel rebuilt,
// a work buffer grown.
enum OverlapWait { kOverlapNoWait = 0, kOverlapStreamWait = 1, kOverlapHostWait = 2 };
struct OverlapChange {
    bool pkeys_rebuilt, cull_fresh, cull_replaced, jit_rebuilt, buffer_grown;
};
OverlapWait overlap_wait(const OverlapChange& c);

// A band set (band, stride, offset) is frame rows {y : (y / band) % stride == offset}.
int band_set_rows(int H, int band, int stride, int offset);
int band_slot_rows(int H, int band, int stride); // largest band set of the split
void scatter_band_set(const unsigned char* slot, size_t plane, int W, int H, int band, int stride, int offset,
                      rt_color* sum_rgb, uint32_t* samples, uint32_t* misses);

} // namespace rtc
