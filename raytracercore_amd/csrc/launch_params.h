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

// A band set (band, stride, offset) is frame rows {y : (y / band) % stride == offset}.
int band_set_rows(int H, int band, int stride, int offset);
int band_slot_rows(int H, int band, int stride); // largest band set of the split
void scatter_band_set(const unsigned char* slot, size_t plane, int W, int H, int band, int stride, int offset,
                      rt_color* sum_rgb, uint32_t* samples, uint32_t* misses);

} // namespace rtc
