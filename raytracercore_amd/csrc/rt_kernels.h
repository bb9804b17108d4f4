// rt_kernels.h -- launch interface between the C ABI (rtcore_api.hip) and the kernels.
#pragma once
#include "../../include/rtcore_rng.h"
#include "rt_internal.h"

namespace rtc {

constexpr int kMaxSplit = 8;     // item ranges of a launch: one per XCD of the MI355X
constexpr int kSplitStride = 32; // dispenser words apart (one 128-B line each)

// Where the work items of a path launch come from (refill, kernels_path.hip): the pixels of a window,
// a caller's rays (rt_render_rays), a list of frame pixels (rt_render_pixels), a caller's beams
// (rt_render_beams) or a caller's surfels (rt_render_surfels).
enum ItemSource : int { ITEMS_TILE = 0, ITEMS_RAYS = 1, ITEMS_PIXELS = 2, ITEMS_BEAMS = 3, ITEMS_SURFELS = 4 };

// Work decomposition of one path-tracing launch over a w x h tile.
struct PathParams {
    int x0, y0, w, h;           // tile within the frame
    int band;                   // band > 0: tile row r is frame row
                                // y0 + ((r / band) * band_stride + band_offset) * band + r % band
    // rt_render_list, the RAYS, BEAMS and SURFELS instances with an index list (index_list below; a list
    // launch has no band, band = 0, so its two words carry the list's): the records the entries name, and
    // whether entry j's record lies at list position j (1: the host entry's gathered chunk) or at its
    // entry number index_list[j] (0: the device entry's resident array)
    union {
        int band_stride;
        unsigned int n_records;
    };
    union {
        int band_offset;
        int list_gathered;
    };
    int band_log2;              // log2(band) for a power-of-two band, else -1 (divide by inv_band)
    float inv_band;             // fp32 1 / band
    int spp;                    // samples per pixel in this launch
    int chunk;                  // samples per work item (a lane owns one item at a time)
    int n_chunks;               // ceil(spp / chunk) rounded up to a power of two: the chunk field of the item
    int log2_chunks;            // index; the slots past the real chunks are never dealt (ticket_items below)
    int blocks_x;               // 8x8 pixel blocks per tile row
    int n_pad;                  // padded pixels per chunk (blocks * 64)
    int refill;                 // BVH kernel: waiting lanes (of 64) that trigger the shading phase
    int spec;                   // BVH kernel (walk_step): lanes blocked on a pending leaf that trigger a leaf step
    int pool;                   // work items a wave takes per atomic: 64 x a power of two <= n_chunks
                                // (all from one 8x8 block, so a wave's lanes stay on neighbouring pixels)
    float inv_blocks_x;         // fp32 reciprocal for the item decode (when magic_bx == 0)
    unsigned magic_bx;          // ceil(2^32 / blocks_x) when block / blocks_x = umulhi(block, magic_bx) for
                                // every block of the launch (make_params checks), else 0
    unsigned long long seed;
    rt_key2 seed_key;           // rt_rng_seed_key(seed) (rtcore_rng.h)
    unsigned long long sample_base;
    const rt_key2* pkeys;       // brute-force kernels: rt_rng_pixel_key(seed_key, pixel) per frame pixel
                                // (cached per scene and seed, pixel_keys_kernel), or null: hashed per item
    unsigned int* counter;      // work-item dispensers (zeroed before launch), one per item range, kSplitStride apart
    int n_split;                // item ranges (1 or kMaxSplit): range g = blocks [split_start[g], split_start[g + 1])
                                // in item units, dealt first to the workgroups b with b % n_split == g (the
                                // workgroups that share one XCD and its L2), then to any wave once theirs is spent
    unsigned split_start[9];
    // The dispensers count tickets, one per atomic (ticket_items below maps a ticket to its items).
    // Per 8x8 block: tpb tickets of p.pool items over the block's first tpb * pool / 64 chunks, all
    // full-length; then one ticket of tail_len items from chunk tail_first / 64 on, the rest of the
    // block's real chunks with the short last chunk among them (tail_len 0: there is no such rest).
    // A range deals the first kind for all its blocks (split_full[g] tickets), then the second.
    unsigned tpb;               // tickets of the first kind per block
    unsigned magic_tpb;         // ceil(2^32 / tpb): t / tpb = umulhi(t, magic_tpb) for every ticket of the
                                // launch (make_params checks); 0 for tpb <= 1
    unsigned tail_first;        // first item of a block's last ticket, relative to the block's first item
    unsigned tail_len;          // its items (64 x its chunks, at most p.pool)
    int linear;                 // 1: every slot is dealt and none is short (tail_len 0, tpb * pool = 64 * n_chunks),
                                // so ticket t of range g is the p.pool items from split_start[g] + t * pool, which
                                // the kernels then take without ticket_items
    int batch;                  // brute-force kernels: lanes that must wait for an item before a wave whose pool
                                // is used up draws its next ticket (0: no waiting; 64: the wave opens a ticket's
                                // items together)
    unsigned split_full[8];     // range g: tickets of the first kind
    unsigned split_tickets[8];  // range g: tickets in all (the dispenser value at which it is spent)
    float4* partial;           // [block][chunk][64 pixels]: rgb sums, (samples | misses << 16)
    unsigned long long* rays;   // Scene.RayTrace-equivalents (added to)
    int* stack_ovf;             // BVH kernels: traversal-stack overflow, RT_STACK_OVF entries per lane of the grid
    unsigned long long* stats;  // optional [7]: node visits, triangle tests, sphere tests (per lane);
                                //   wave cycles in sample start, traversal, shading; wave iterations
    // The scene as this launch's kernel variant walks it (fill_launch).  The brute-force kernels read
    // these from the launch record by scalar loads where they are used, instead of holding them in
    // SGPRs as kernel arguments for the whole kernel (which spilled into VGPR lanes).
    PathScene scene;
    const TestRec* tests;
    const float4* rows;         // BVH kernels: 3 float4 per slot, the compact leaves' records (DevScene::rows_bvh)
    const RectRec* rects;
    const FrameRec* frames;
    const PrimF* prims;
    const GroupRec* groups;
    const NodeF* nodes;         // BVH kernels: the BVH2 and the wide tree
    const Node4Q* nodes4;
    const XformF* xf;
    const MatF* mats;
    const float4* vnormals;
    const PrimD* prims_d;       // the exact fp64 records by primitive ID (the vertex-normal re-hit test)
    float4* ray_log;            // BVH kernels, instrumented launch only (rt_debug_ray_log): every finished
    unsigned int* ray_log_n;    //   query as 3 float4 (o, prev | d | t, sg) appended at ray_log_n, up to
    unsigned int ray_log_cap;   //   ray_log_cap records
    // rt_trace_paths, instrumented launch only (null on every other launch): one rt_debug_ray per
    // bounce as kRecRows float4, record ((py * w + px) * spp + sample) * (recursion + 1) + bounce of the
    // tile (row-major over the tile, like the other device buffers), and one float4 per sample when
    // it ends: its colour as rt_render_tile_1spp returns it, and the number of its records
    float4* rec_rays;
    float4* rec_samples;
    unsigned int rec_max;       // records in rec_rays (no store at or past it)
    // rt_render_rays, the RAYS instances only (null / 0 on every other launch; last, so that no other
    // field moves): the caller's rays as rt_ray rows.  The launch is planned as a tile 8 pixels wide
    // (make_params_rays), so the 64 items of block b and one chunk are the rays 64 b .. 64 b + 63: ray
    // i = (block << 6) | pixel of the item, and its pixel key is that of stream_base + i.
    // rt_render_pixels, the PIXELS instances only: the launch is planned in the same way
    // (make_params_pixels), entry i = (block << 6) | pixel of the item names the frame pixel
    // pixel_list[i] = fy * scene.width + fx, and an entry at or past n_frame_px is skipped.  The list's
    // fields share the rays' storage, so that the record keeps its size and no field moves: the kernels
    // that take it by value are as they were.
    // rt_render_beams, the BEAMS instances only: the launch is planned as for the rays, and entry i of
    // beam_list is an rt_beam as twelve rows (rt_beam.h); the pointer shares the rays' storage too.
    // rt_render_surfels, the SURFELS instances only: the launch is planned as for the rays, and entry i
    // of ray_list is an rt_surfel as four rows (position, normal; rt_surfel.h).  gather_mode, the
    // rt_gather_mode of the launch, shares start_rows' word: a list launch has no start rows.
    // Start rows, the brute-force tile instances only (run_path plans them, plan_start_rows; null / 0:
    // off): float4 starts[wave][start_rows][64], wave = blockIdx.x * 4 + threadIdx.x / 64 of the
    // persistent grid, start_rows = chunk.  A wave that opens items writes every camera sample of a
    // lane's item as one row (direction xyz, the rng after GetCameraRay's two draws), all lanes
    // together; a lane's sample start reads its own row back (refill).  The pointer shares the lists'
    // storage (a tile launch has no list) and the count takes the padding after n_rays, so that the
    // record keeps its size and no field moves.
    union {
        const double2* ray_list;    // four 16-B rows per ray (origin xy, origin zw, direction xy, direction zw)
        const uint32_t* pixel_list; // frame pixel indices
        const double2* beam_list;   // twelve 16-B rows per beam (rt_beam: origin, direction, their steps in u and v)
        float4* starts;
    };
    unsigned int n_rays;        // rays or list entries of the launch (the items of the last block past it stay closed)
    union {
        int start_rows;
        int gather_mode;
    };
    union {
        unsigned long long stream_base;
        struct {
            unsigned int n_frame_px; // scene.width * frame height
            float inv_frame_w;       // fp32 1 / scene.width (list_pixel)
        };
    };
    int scene_bound;            // flat brute-force kernel: 1 = a wave of camera rays that all miss the scene bound
                                // skips its query (RTCORE_SCENE_BOUND, make_params_for)
    // Sample rounds, the brute-force tile instances only (refill; RTCORE_SAMPLE_ROUNDS, make_params_for):
    // 0 no ticket runs in rounds, 2 every ticket, 1 those ticket_rounds below picks.  It takes the
    // padding after scene_bound, so that the record keeps its size and no field moves.
    int sample_rounds;
    // The block cull (block_cull.h, run_path): null, or a device record of the launch's 8x8 blocks whose
    // pixels can see the scene.  The launch is then planned over those live blocks alone, numbered
    // 0 .. n_live - 1 in their original order (n_pad = 64 n_live; blocks_x stays the window's):
    //   words 0-1  the real pixels of the dead blocks (64 bits; each stands for spp primary misses and rays)
    //   word  2-3  n_live, blocks of the window
    //   kCullTable + i             live block i -> bx | by << 16
    //   kCullTable + n_live + b    window block b = by * blocks_x + bx -> its live number, or -1
    // One field (last, so that no other moves): the BVH kernels take this record by value.
    // rt_render_list, the RAYS, BEAMS and SURFELS instances (a list launch has no cull): null, or the index
    // list.  Item j = (block << 6) | pixel then names entry e = index_list[j]: its stream key is that
    // of stream_base + e, its record is e's (or j's, list_gathered), and an entry at or past n_records
    // opens no item.  Null on rt_render_rays', rt_render_beams' and rt_render_surfels' own launches.
    union {
        const unsigned int* cull;
        const unsigned int* index_list;
    };
};
static_assert(__builtin_offsetof(PathParams, start_rows) == __builtin_offsetof(PathParams, n_rays) + 4 &&
                  __builtin_offsetof(PathParams, scene_bound) == __builtin_offsetof(PathParams, n_rays) + 16,
              "start_rows takes the padding after n_rays");
static_assert(__builtin_offsetof(PathParams, sample_rounds) == __builtin_offsetof(PathParams, scene_bound) + 4 &&
                  __builtin_offsetof(PathParams, cull) == __builtin_offsetof(PathParams, scene_bound) + 8,
              "sample_rounds takes the padding after scene_bound");
constexpr int kCullTable = 4;  // first table word of PathParams::cull

// First bounce (path_body, the flat brute-force tile instances that run sample rounds; RTCORE_FIRST_BOUNCE,
// make_params_for).  Two more bits of PathParams::scene_bound, whose bit 0 is the scene bound's switch:
//   kFirstBounce  the switch: the launch may use unit masks
//   kFirstMasks   it has them: its cull record ends with one 64-bit unit mask per live block (run_path)
// The flat order's test units, in the order trace_brute runs its one group: each world rectangle (x | y |
// z), each world box, each frame (its rectangles and its box together), each triangle record, each
// sphere record.  Bit u of a block's mask is clear when no camera ray of the block can meet unit u
// (unit_masks, block_cull.h); the masks follow the cull record's two tables, on an 8-byte boundary.
constexpr int kFirstBounce = 2, kFirstMasks = 4;
constexpr int kMaxUnits = 64;
template <class GroupT>
__host__ __device__ inline int flat_unit_count(const GroupT& G)
{
    return G.n_rect[0] + G.n_rect[1] + G.n_rect[2] + G.n_boxes + G.n_frames + (G.n_tri_sph & 0xFFFF) + (G.n_tri_sph >> 16);
}
__host__ __device__ inline unsigned cull_masks_at(unsigned n_live, unsigned n_blocks) // first mask word
{
    return ((unsigned)kCullTable + n_live + n_blocks + 1u) & ~1u;
}
constexpr int kRecRows = 6;    // sizeof(rt_debug_ray) / 16

// Ticket t of item range g -> the items it covers, [first, first + len) in the item numbering
// ((block << log2_chunks) + chunk) * 64 + pixel: chunks of one 8x8 block next to each other, none
// past the launch's real chunks.  t < p.split_tickets[g].  The kernels' refill and the host check
// (rt_debug_item_order) both call this; every operand is wave-uniform in the kernels.
template <class ParT>
__host__ __device__ inline void ticket_items(const ParT& p, unsigned g, unsigned t, unsigned& first, unsigned& len)
{
    const unsigned full = p.split_full[g];
    unsigned blk, off;
    if (t < full) {
        blk = p.magic_tpb ? (unsigned)(((unsigned long long)t * p.magic_tpb) >> 32) : t;
        off = (t - blk * p.tpb) * (unsigned)p.pool;
        len = (unsigned)p.pool;
    } else {
        blk = t - full;
        off = p.tail_first;
        len = p.tail_len;
    }
    first = p.split_start[g] + (blk << (p.log2_chunks + 6)) + off;
}

// Sample rounds: does the ticket a wave draws now run in rounds (refill holds every lane at its
// sample's end until no lane of the wave is live, so that the wave starts its samples together)?
// Rounds cost no wave iteration where the paths of a ticket are equally long, and many where they
// are not, so a wave chooses per ticket, from what its previous ticket was like.  first: the wave has
// had no ticket yet, and runs this one free.  prev_rays: the rays the wave traced since it drew its
// previous ticket.  Rounds when that ticket's paths nearly all ran to the recursion limit, at least
// kRoundsNum / kRoundsDen of pool x chunk samples x (recursion + 1) rays (bounce.txt: a closed room).
// A ticket whose samples all missed says nothing about the next one: rounds after it as well cost
// die.txt's silhouette blocks their ragged paths (die4k +0.5 %, DESIGN appendix A) and bought
// bounce.txt nothing.  A short last ticket counts against the full one, so it can only fall below
// the bound.  The ray count
// is taken modulo 2^32; a ticket has fewer rays than that up to recursion 16383, and past it the
// choice, never a result, may go wrong.  Wave-uniform in the kernels; the host check
// (tests/host/rounds_rule_check.cpp) calls it too.
constexpr unsigned kRoundsNum = 4, kRoundsDen = 5; // T = 0.8 (tools/round_sim.py)
template <class ParT>
__host__ __device__ inline bool ticket_rounds(const ParT& p, int recursion, bool first, unsigned prev_rays)
{
    if (p.sample_rounds != 1) return p.sample_rounds == 2;
    if (first) return false;
    const unsigned long long samples = (unsigned long long)(unsigned)p.pool * (unsigned long long)(unsigned)p.chunk;
    return (unsigned long long)prev_rays * kRoundsDen >= samples * (unsigned long long)(unsigned)(recursion + 1) * kRoundsNum;
}

// Trace-only kernel over a ray list (rt_debug_trace_rays): the wide BVH's speculative traversal
// without the shading phase, for measuring what a wavefront split's traversal stage would take.
struct TraceRaysParams {
    const float4* rays;         // 3 float4 per ray as the ray log writes them
    float2* hits;               // (t, bitcast sg) per ray
    unsigned int n;
    unsigned int* counter;      // ray dispenser (zeroed before the launch)
    int* stack_ovf;
    const TestRec* tests;
    const float4* rows;
    const Node4Q* nodes4;
    const XformF* xf;
    int root4;
    int spec;                   // blocked lanes that trigger a leaf step (as PathParams.spec)
    const GroupRec* outer;      // the BVH order's outer group (DevScene::groups_bvh) or null
    const RectRec* outer_rects;
    const FrameRec* outer_boxes;
    unsigned long long* stats;  // optional [3]: node visits, leaf-step lane slots, lane slots in all
};

#ifndef __HIPCC_RTC__ // host-side launch interface (not part of a hiprtc-compiled kernel)
// Closest-hit queries over caller-supplied rays (rt_query_rays, RT_QUERY_FAST): the scene as the
// generic path kernel of the traversal mode walks it (fill_launch; the wide tree from its global
// nodes, without the hot table) and the ray and hit arrays.
struct QueryParams {
    const double2* rays;        // rt_ray: four 16-B rows (origin xy, origin zw, direction xy, direction zw)
    float4* hits;               // rt_hit: three 16-B rows
    unsigned int n;
    unsigned int* counter;      // BVH kernel: ray dispenser (zeroed before the launch)
    int* stack_ovf;             // BVH kernel: traversal-stack overflow area
    PathScene scene;            // n_groups, n_bvh, n_pln, facts (the brute-force orders; the BVH order's outer group)
    const TestRec* tests;
    const float4* rows;
    const RectRec* rects;
    const FrameRec* frames;
    const PrimF* prims;
    const GroupRec* groups;
    const Node4Q* nodes4;
    const XformF* xf;
    const float4* vnormals;
    int root4;
    int n_nodes4;               // wide nodes (0: root4 names a leaf, or the scene holds only planes)
    int spec;                   // BVH kernel: blocked lanes that trigger a leaf step (as PathParams.spec)
};
constexpr int kHitRows = 3;     // sizeof(rt_hit) / 16

// rt_query_rays: kernel 0 brute force, 1 grouped brute force, 3 the wide BVH (the numbering of
// path_variant).  query_blocks_per_cu: blocks of 256 per CU the kernel can hold; the brute-force
// kernels take any grid (grid-stride loop), the BVH kernel deals rays to whatever grid it gets.
int query_blocks_per_cu(int kernel);
hipError_t launch_query(const QueryParams& p, int kernel, int grid_blocks, hipStream_t stream);
// RT_QUERY_EXACT (kernels_exact.hip): the fp64 reference query, one ray per lane; prim_id -2 where
// the reference BVH is deeper than the kernel's traversal stack.
hipError_t launch_query_exact(const DevScene& s, const rt_ray* d_rays, unsigned n, rt_hit* d_hits, hipStream_t stream);
// rt_occluded_rays: the scene and the rays as rt_query_rays' kernels take them (q.hits unused), the
// segments' ends and one answer byte per ray.
struct OccludedParams {
    QueryParams q;
    const double* t_max;        // per ray, or null: +inf for every ray
    unsigned char* out;         // 0 / 1 per ray (RT_QUERY_EXACT: 255 on a traversal-stack overflow)
    int early;                  // 1: the planes (BVH: and the outer records) are tested before the other records,
                                // 0: after them (BVH: only when the tree gave no hit)
};
// RT_QUERY_FAST: kernel numbering, grids and blocks per CU as launch_query / query_blocks_per_cu.
int occluded_blocks_per_cu(int kernel);
hipError_t launch_occluded(const OccludedParams& p, int kernel, int grid_blocks, hipStream_t stream);
// rt_occluded_surfels: the scene as rt_occluded_rays' kernels take it, q.rays the surfel records (an
// rt_surfel has an rt_ray's rows) and q.n the list positions of the launch (q.hits unused).  Entry e of
// position j is index[j], or j without a list; the records, t_max and the counts are indexed by entry.
struct OccludedSurfelsParams {
    QueryParams q;
    const unsigned int* index;  // list positions -> entries, or null: the identity
    unsigned int n_records;     // entries at or past it are skipped
    const double* t_max;        // per entry, or null: +inf for every entry
    unsigned int* occluded;     // per entry, added to
    unsigned int* samples;      // per entry, added to, or null
    int early;                  // as OccludedParams.early
    int gather_mode;            // rt_gather_mode
    unsigned int spp;           // samples of the launch per entry
    unsigned int log2_lanes;    // brute force: lanes that share a list position, 1 << log2_lanes <= 64
    unsigned int block;         // brute force: samples of one work unit ((64 >> log2_lanes) positions x block samples)
    unsigned int blocks;        // brute force: units per position, ceil(spp / block); 1: its lanes own its entry
    unsigned int refill;        // BVH: lanes without a query that trigger a refill (1 ... 64)
    rt_key2 seed_key;
    unsigned long long sample_base, stream_base;
};
// Kernel numbering as launch_occluded.  The brute-force kernels take any grid (grid-stride loop over the
// units, one wave per unit), the BVH kernel deals q.n * spp (position, sample) units to whatever grid it gets.
int occluded_surfels_blocks_per_cu(int kernel);
hipError_t launch_occluded_surfels(const OccludedSurfelsParams& p, int kernel, int grid_blocks, hipStream_t stream);
// RT_QUERY_EXACT (kernels_exact.hip): ref_raytrace_hit's distance against t_max in fp64, one ray per lane.
hipError_t launch_occluded_exact(const DevScene& s, const rt_ray* d_rays, const double* d_t_max, unsigned n,
                                 unsigned char* d_out, hipStream_t stream);
// Sets p.scene and the record pointers of the given kernel variant's slot order.
void fill_launch(const DevScene& s, int variant, PathParams& p);

// mode 0: primary hit IDs, mode 1: reference-BVH node counts (DebugRaycaster BoundingVolumes)
hipError_t launch_primary_ids(const DevScene& s, const CameraD& cam, int x0, int y0, int w, int h, int mode,
                              int32_t* d_ids, hipStream_t stream);

// DebugRaycaster Selection mode (kernels_exact.hip): the fold of rt_exact_prims.h's select_items over
// n_items device-resident items, for the camera's pixels of a tile (d_out row-major, y*w + x) or for
// n <= 2^32 - 64 caller-supplied rays (d_out by ray).
hipError_t launch_select_pixels(const DevScene& s, const CameraD& cam, const rt_select_item* d_items, int n_items, int x0,
                                int y0, int w, int h, rt_selection* d_out, hipStream_t stream);
hipError_t launch_select_rays(const DevScene& s, const rt_select_item* d_items, int n_items, const rt_ray* d_rays,
                              unsigned n, rt_selection* d_out, hipStream_t stream);

// Kernel variant: kernel 0 brute force, 1 grouped brute force, 2 BVH2 (24-entry stack), 3 wide BVH
// (RT_WIDE_STACK = 16-entry stack), both + kStackOverflow entries in global memory;
// lds stages the shading records in LDS.
int path_variant(int kernel, bool lds);
constexpr int kStackOverflow = 44; // (rt_trace.h asserts that the kernels' RT_STACK_OVF is the same)
constexpr int kTestSpares = 3;     // zero TestRecs after the BVH-order records (leaf steps of up to 4 loads)
int path_wide_stack();              // LDS entries of the wide BVH kernel's stack (RT_WIDE_STACK)
size_t path_lds_bytes(const DevScene& s);   // dynamic LDS of the staged (lds) variants
size_t path_dyn_lds(const DevScene& s, int variant); // all dynamic LDS of a variant (+ the wide kernel's hot nodes)
// Launch the persistent kernel; stats counts node visits / primitive tests (slower build).
// The camera and the launch parameters are read from device memory (d_cam, d_params).
// src: ITEMS_RAYS, rt_render_rays' instance of the variant (PathParams::ray_list), which does not read
// the camera; ITEMS_PIXELS, rt_render_pixels' (PathParams::pixel_list); ITEMS_BEAMS, rt_render_beams'
// (PathParams::beam_list, no camera either); ITEMS_SURFELS, rt_render_surfels' (ray_list as rt_surfel
// rows and PathParams::gather_mode, no camera).  All exist for the brute-force and the wide BVH kernels
// and are never instrumented.
hipError_t launch_path(const DevScene& s, const CameraF* d_cam, const PathParams* d_params, int variant,
                       int grid_blocks, hipStream_t stream, bool stats, ItemSource src = ITEMS_TILE);
// Blocks of 256 threads a CU can hold of a kernel, at least 1 (also when the runtime cannot say).
template <class KernelT>
inline int blocks_per_cu(KernelT kernel, size_t dyn_lds = 0)
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void*>(kernel), 256, dyn_lds) != hipSuccess ||
        n < 1)
        n = 1;
    return n;
}
// vn: scene has vertex-normal triangles
int path_blocks_per_cu(int variant, size_t dyn_lds, bool stats, bool vn, ItemSource src = ITEMS_TILE);
// The trace-only kernel (waves per SIMD 6 / 7 / 8 with LDS stacks of 20 / 16 / 16 entries): blocks
// per CU and launch (grid blocks of 256).
int trace_rays_blocks_per_cu(int waves);
// Host evaluation of the kernels' vertex-normal re-hit test (vn_rehit_test): Triangle.RayTraceAVXFaster
// in fp64 from the hit point fma(e01, u, fma(e02, v, v0)) along dir; returns 1 on a hit, with its
// Inside flag, t and the origin used.
int debug_vn_rehit(const double v0[3], const double e01[3], const double e02[3], int mirror, double u, double v,
                   const float dir[3], int* inside, double* t, double o[3]);
hipError_t launch_trace_rays(const TraceRaysParams& p, int waves, int grid_blocks, hipStream_t stream);
// out[y * w + x] = rt_rng_pixel_key(seed_key, y * w + x) for a w x h frame
hipError_t launch_pixel_keys(rt_key2 seed_key, int w, int h, rt_key2* out, hipStream_t stream);
// The BVH order's rows (3 float4 per record, n_records including the spares) from its TestRecs and,
// with rewrite, every homogeneous leaf reference of the BVH2 and the wide tree made compact
// (rt_internal.h, kLeafCompact).
hipError_t compact_leaves(const TestRec* d_tests, int n_records, float4* d_rows, NodeF* d_nodes, int n_nodes,
                          Node4Q* d_nodes4, int n_nodes4, bool rewrite, hipStream_t stream);

// partial -> fp64 planar accumulators (d_sum planes R | G | B, each `plane` doubles apart;
// 0 = w*h), d_samples, d_misses (row-major w*h), added to.  d_set_rays (an overlapped launch): the
// launch set's ray counter, moved into d_rays and zeroed.
hipError_t launch_accumulate(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                             hipStream_t stream, size_t plane = 0, unsigned long long* d_set_rays = nullptr,
                             unsigned long long* d_rays = nullptr);
// SampleSet.GetOutput over planar accumulators (row-major w*h) -> ARGB codes.
hipError_t launch_tonemap(int w, int h, const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses,
                          rt_color back, double back_alpha, double exposure, int32_t* d_argb, hipStream_t stream);
// One pixel of the host-buffer entry point's layout (rt_render_tile): the accumulated DoubleColor,
// samples and misses, in the caller's x*h + y order.
struct TileRec {
    double r, g, b;
    uint32_t samples, misses;
};
// rt_render_rays: a RAYS launch's partials folded per ray, in chunk order.  d_recs null: added to
// d_sum (planes R | G | B of p.n_rays doubles), d_samples, d_misses; else written to d_recs[p.n_rays].
hipError_t launch_accumulate_rays(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                  TileRec* d_recs, hipStream_t stream);
// rt_render_pixels: a PIXELS launch's partials (at accumulate_rays_kernel's addresses) folded per list
// entry, in chunk order, into whole-frame accumulators at pixel_list[i] (row-major, planes `plane`
// apart, as launch_accumulate), added to; d_q and d_batches (both or neither) get the moments of
// rtcore.h's "adaptive sampling".  An entry outside the frame is skipped.
hipError_t launch_accumulate_pixels(const PathParams& p, double* d_sum, uint32_t* d_samples, uint32_t* d_misses,
                                    double* d_q, uint32_t* d_batches, size_t plane, hipStream_t stream);
// One list entry of rt_render_pixels' host entry: what the fold adds to the entry's pixel.
struct PixelRec {
    double r, g, b, q;
    uint32_t samples, misses, batches, pad;
};
// The same fold from zero, one PixelRec per entry (q and batches always)
hipError_t launch_accumulate_pixels_recs(const PathParams& p, PixelRec* d_recs, hipStream_t stream);
// rt_render_list: a RAYS, BEAMS or SURFELS launch's partials folded per list position i, in chunk order,
// into per-entry accumulators at e = d_index[i] (null: i), planes `plane` apart (0 = n_records), with
// launch_accumulate_pixels' moments; an entry at or past n_records is skipped.  d_recs: instead written
// from zero as one PixelRec per list position.
hipError_t launch_accumulate_list(const PathParams& p, const uint32_t* d_index, size_t n_records, double* d_sum,
                                  uint32_t* d_samples, uint32_t* d_misses, double* d_q, uint32_t* d_batches, size_t plane,
                                  PixelRec* d_recs, hipStream_t stream);
// One probe of rt_render_probes' host entry: the accumulators as they travel, up with what the caller's
// arrays hold in sh and zero counts, down with the call's samples folded in.
struct ProbeRec {
    rt_probe_sh sh;
    uint32_t samples, misses;
};
// rt_render_probes: the partials of a SURFELS launch in RT_GATHER_SPHERE planned by make_params_probes (one
// sample per work item) folded per probe in sample order, each sample weighted by the L2 basis (rt_sh.h) of
// its direction, which the fold draws again as the launch did (p.ray_list, the seed and the bases of p).
// d_recs null: added to d_sh, d_samples, d_misses (p.n_rays each); else to d_recs[p.n_rays] in place.
hipError_t launch_accumulate_probes(const PathParams& p, rt_probe_sh* d_sh, uint32_t* d_samples, uint32_t* d_misses,
                                    ProbeRec* d_recs, hipStream_t stream);
// rt_render_probe_list: launch_accumulate_probes for a launch with an index list over n_records resident
// records (d_index null: the identity): list position i's samples go into d_sh, d_samples, d_misses and, where
// given, d_moments (rt_probe_error.h) at the entry d_index[i]; an entry at or past n_records is skipped.
hipError_t launch_accumulate_probe_list(const PathParams& p, const uint32_t* d_index, size_t n_records, rt_probe_sh* d_sh,
                                        uint32_t* d_samples, uint32_t* d_misses, rt_probe_moments* d_moments,
                                        hipStream_t stream);
// planar row-major accumulators (w*h) -> TileRec[w*h] in x*h + y order
hipError_t launch_tile_host_layout(int w, int h, const double* d_sum, const uint32_t* d_samples,
                                  const uint32_t* d_misses, TileRec* d_out, hipStream_t stream);
// rt_trace_paths: a launch's records (PathParams::rec_rays, kRecRows * (recursion + 1) float4 per
// sample) and per-sample rows (rec_samples), row-major over the tile -> the caller's order
// (x*h + y) * spp + k.
hipError_t launch_trace_host_layout(int w, int h, int spp, int recursion, const float4* d_rays, const float4* d_samples,
                                    float4* d_rays_out, float4* d_samples_out, hipStream_t stream);
// partial (1 spp) -> the DoubleColor[w, h] values as fp32 rgb in x*h + y order, Placeholder(-1) on a miss.
hipError_t launch_colors_1spp(const PathParams& p, float* d_out, hipStream_t stream);

#endif

} // namespace rtc
