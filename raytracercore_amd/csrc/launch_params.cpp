// launch_params.cpp -- host-side launch planning (launch_params.h).
#include "launch_params.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "host_scene.h"

namespace rtc {

// The order in which the dispensers deal p's work items (PathParams::tpb .. split_tickets, ticket_items
// in rt_kernels.h), from p's chunks, pool and ranges.  Only which wave takes which item depends on it.
// A pixel's real chunks are the first `used` of the n_chunks slots of the item index; the last of
// them is short when chunk does not divide spp.  Per range, every block's full-length chunks are
// dealt first, p.pool / 64 of them per ticket, then one shorter ticket per block with what is left:
// the full chunks that do not fill a ticket and the short chunk.  The launch then ends on its
// shortest items, and no ticket names a chunk slot past `used`.  A ticket is always adjacent chunks
// of one block, whatever the chunks and the pool.  With every slot real and no short chunk (C1, C4
// at 64 spp) the tickets are p.pool items each in index order: the sequence before tickets were
// introduced.  RTCORE_ITEM_ORDER=0 deals all n_chunks slots that way (A/B), and so does a launch
// with so many tickets that the division below would not be exact.
// Measured, 1080p, kernel ms, one call each (profiles/r07): without the waves' batched item opening
// (RTCORE_ITEM_BATCH=0, below) this order is the slower one, C2 16.64 -> 16.78, C3 20.80 -> 21.51:
// a wave that drew a ticket of empty slots had its waiting lanes open the next ticket together, a
// little of what the batching now does outright.  With the batching the empty slots only cost:
// C2 16.07 -> 16.01, C3 20.19 -> 20.10 with this order.
void set_item_order(PathParams& p)
{
    const char* e = getenv("RTCORE_ITEM_ORDER");
    bool dense = !(e && e[0] == '0');
    const unsigned slots = (unsigned)p.pool / 64u; // chunks per ticket: a power of two <= n_chunks
    const unsigned used = (unsigned)((p.spp + p.chunk - 1) / p.chunk);
    const unsigned n_blocks = (unsigned)(p.n_pad / 64);
    for (;; dense = false) {
        const unsigned n_real = dense ? used : (unsigned)p.n_chunks;
        const unsigned n_full = dense && p.spp % p.chunk != 0 ? used - 1 : n_real;
        p.tpb = n_full / slots;
        p.tail_first = p.tpb * (unsigned)p.pool;
        p.tail_len = (n_real - p.tpb * slots) * 64u; // <= pool: at most slots - 1 full chunks and the short one
        // t / tpb by multiply-high, as magic_bx: exact for every t with t * (M * tpb - 2^32) < 2^32,
        // M = ceil(2^32 / tpb); t < n_blocks * tpb.  (A power of two has M * tpb = 2^32, so the
        // RTCORE_ITEM_ORDER=0 form always passes.)
        p.magic_tpb = 0;
        if (p.tpb <= 1) break;
        const uint64_t M = ((1ull << 32) + p.tpb - 1) / p.tpb;
        const uint64_t err = M * p.tpb - (1ull << 32);
        if (M < (1ull << 32) && (uint64_t)n_blocks * p.tpb * err < (1ull << 32)) {
            p.magic_tpb = (unsigned)M;
            break;
        }
    }
    p.linear = p.tail_len == 0 && p.tpb * slots == (unsigned)p.n_chunks;
    for (int g = 0; g < kMaxSplit; g++) {
        const unsigned b = g < p.n_split ? (p.split_start[g + 1] - p.split_start[g]) >> (p.log2_chunks + 6) : 0u;
        p.split_full[g] = b * p.tpb;
        p.split_tickets[g] = p.split_full[g] + (p.tail_len ? b : 0u);
    }
}

// The launch's blocks, item ranges and tickets for n_blocks 8x8 blocks numbered 0 .. n_blocks - 1:
// the window's own (make_params_for), or the live blocks of a culled launch (run_path, block_cull.h),
// whose chunks, samples per item and pool stay the window's, so that an item holds the same samples.
void set_blocks(PathParams& p, int n_blocks)
{
    p.n_pad = n_blocks * 64;
    p.n_split = 1;
    int want = kMaxSplit;
    if (const char* e = getenv("RTCORE_XCD_SPLIT")) want = atoi(e) > 0 ? kMaxSplit : 1;
    if (want > 1 && n_blocks >= 4 * kMaxSplit) p.n_split = kMaxSplit;
    for (int g = 0; g <= p.n_split; g++)
        p.split_start[g] = (unsigned)((int64_t)n_blocks * g / p.n_split) * (unsigned)(p.n_chunks * 64);
    set_item_order(p);
}

// chunk_npix (default w * h): the pixel count the chunks per pixel are chosen for.  A column band of a
// tile passes the whole tile's, so that every pixel's samples fall into the same chunks (and its
// fp64 sum into the same order) as in one launch over the tile.
// kernel: 0 flat, 1 grouped brute force, 2 / 3 the BVH kernels; chunks_over / pool_over > 0 (the host
// check, rt_debug_item_order): chunks per pixel and items per ticket instead of the tuned ones.
PathParams make_params_for(int kernel, int chunks_over, int pool_over, int x0, int y0, int w, int h, int spp,
                           uint64_t seed, uint64_t base, double chunk_npix)
{
    PathParams p{};
    p.x0 = x0;
    p.y0 = y0;
    p.w = w;
    p.h = h;
    p.band = 0;
    p.spp = spp;
    // a few chunks per pixel keep the tail of a launch short while each lane still amortises
    // its item fetch over many samples (RTCORE_PATH_CHUNKS overrides the count, for tuning).
    // A launch over fewer pixels than a 1080p frame takes proportionally more chunks per pixel
    // (up to 8 x the base count: 192 for the brute-force kernels, 512 for the BVH kernels; the
    // partial buffer is 16 B x chunks x padded pixels), so that a band set of 1/N of the frame at N x the samples (bench.py on N GPUs)
    // gets items as short as one GPU's whole-frame launch, and with them the same launch tail.
    // The BVH kernels take twice as many (C4 at 64 spp: one sample per item; 16 / 32 / 64 chunks
    // 58.7 / 55.0-55.2 / 53.7 ms): their items start in batched shading phases, so a short item
    // costs little, and the tail of a launch of long, divergent BVH paths shrinks.
    // Brute-force kernels: 24 chunks (round 6, after the xorshift stream; same call, two rounds,
    // profiles/r06/chunk_sweep3.log, ms per step): C2 16 / 20 / 24 / 28 / 32 chunks 17.12 / 16.86 /
    // 16.84-16.86 / 16.85-16.87 / 16.98; C3 22.16-22.29 / 21.49-21.50 / 21.42-21.43 / 21.43-21.46 /
    // 21.86-21.93.  Fewer, longer items (and fewer partials to fold) until the launch tail grows;
    // 24 chunks leave 8 of the 32 power-of-two chunk slots empty: that sweep still dealt them as items
    // whose lanes sat an iteration out; set_item_order no longer deals them (a re-sweep is due).
    const int base_chunks = kernel >= 2 ? 64 : 24;
    int chunks = base_chunks;
    const double npix = chunk_npix > 0.0 ? chunk_npix : (double)w * (double)h;
    if (npix > 0 && npix < 2073600.0)
        chunks = (int)std::min(8.0 * base_chunks, base_chunks * std::ceil(2073600.0 / npix));
    // A larger frame has more items, so a relatively shorter tail: fewer, longer items then save
    // item switches and partials (die.txt 4K x 512 spp: 8 / 16 / 32 / 64 chunks -> 55.2 / 55.6 /
    // 56.6-57.0 / 57.0 ms kernel, 55.8 / 56.3-56.5 / 57.8-58.1 / 59.0 ms per step).
    else if (npix > 2073600.0)
        chunks = (int)std::max(base_chunks / 4.0, std::ceil(base_chunks * 2073600.0 / npix));
    if (const char* e = getenv("RTCORE_PATH_CHUNKS")) chunks = std::max(1, atoi(e));
    if (chunks_over > 0) chunks = chunks_over;
    p.chunk = std::max(1, std::min(64, (spp + chunks - 1) / chunks));
    const int used = (spp + p.chunk - 1) / p.chunk;
    p.log2_chunks = 0;
    while ((1 << p.log2_chunks) < used) p.log2_chunks++;
    p.n_chunks = 1 << p.log2_chunks; // work items: ((block << log2_chunks) + chunk) * 64 + pixel
    p.blocks_x = (w + 7) / 8;
    p.n_pad = p.blocks_x * ((h + 7) / 8) * 64;
    p.inv_blocks_x = 1.0f / (float)p.blocks_x;
    // Item decode by multiply-high (one v_mul_hi_u32) instead of the fp32-reciprocal divmod: exact
    // for every block index x when x * (M * blocks_x - 2^32) < 2^32, M = ceil(2^32 / blocks_x).
    p.magic_bx = 0;
    if (p.blocks_x > 1 && !getenv("RTCORE_NO_MAGIC_DIV")) { // (the env variable: A/B of the decode)
        const uint64_t M = ((1ull << 32) + (uint64_t)p.blocks_x - 1) / (uint64_t)p.blocks_x;
        const uint64_t err = M * (uint64_t)p.blocks_x - (1ull << 32);
        const uint64_t max_blk = (uint64_t)(p.n_pad / 64);
        if (M < (1ull << 32) && max_blk * err < (1ull << 32)) p.magic_bx = (unsigned)M;
    }
    // One device-scope atomic hands a wave p.pool items.  64 per atomic made the dispenser a
    // bottleneck (measured, 1080p: die.txt grouped 50.9 -> 47.0 ms with 256, 48.2 with 128 or 512;
    // bounce.txt flat 33.4 -> 33.0 ms with 128, 33.6 with 256; mesh BVH 82.2 -> 80.3 with 256).
    // With the XCD-local dispensers (8 words instead of one) smaller pools pay again (round 3, pool
    // multiples 1 / 2 / 4 / 8): flat brute force C2 19.54-19.57 / 19.63-19.69 / 20.05 ms, the BVH
    // kernels C4 44.54-44.57 / 44.25-44.28 / 45.0-45.2 / 46.8 ms; grouped C3 27.81 / - / 27.58-27.64.
    // Round 6, with the 24-chunk items (longer items, so fewer per atomic; profiles/r06/pool_sweep2.log):
    // grouped C3 pool multiples 2 / 4 / 8: 19.93 / 20.36-20.38 / 21.51-21.57 ms; flat C2 1 / 2: 16.27-16.28 /
    // 16.42-16.49 ms.
    int pool_mul = kernel == 0 ? 1 : 2;
    if (const char* e = getenv("RTCORE_POOL_MUL")) pool_mul = std::max(1, std::min(64, atoi(e)));
    if (pool_over > 0) pool_mul = std::max(1, std::min(64, pool_over / 64));
    p.pool = 64;
    while (p.pool < 64 * pool_mul && p.pool < 64 * p.n_chunks) p.pool *= 2;
    // Brute-force kernels: a wave whose pool is used up draws its next ticket only when all 64 lanes
    // wait for an item (refill, kernels_path.hip), so a ticket's items open together and the lanes
    // stay in step; which lane renders an item never changes what it computes.  The iterations in
    // which no lane closes or opens an item branch over those sections, and more lanes share a
    // shading branch.  PMC per launch before this (profiles/r07): where the lanes drifted further
    // apart the same lane work took more wave instructions (C3 +3.75 % VALU instructions at +1.6 %
    // lane cycles).  Kernel ms, 1080p, one call, RTCORE_ITEM_BATCH = 0 / 8 / 16 / 32 / 48 / 64 lanes:
    // C2 16.64 / 16.60 / 16.61 / 16.48 / 16.22 / 16.08, C3 20.87 / 20.70 / 20.62 / 20.45 / 20.25 /
    // 20.15.  Short items gain too (bounce.txt 1080p at 24 / 48 / 96 / 192 spp, 1 / 2 / 4 / 8 samples
    // per item: 2.57 -> 2.53, 3.87 -> 3.73, 6.48 -> 6.08, 12.69 -> 11.96; C1 0.156 -> 0.147).
    // Holding lanes back in the middle of a pool as well (until 4 .. 32 wait) lost 5-19 %.
    p.batch = kernel < 2 ? 64 : 0;
    if (const char* e = getenv("RTCORE_ITEM_BATCH")) p.batch = std::max(0, std::min(64, atoi(e)));
    // Flat brute-force kernel: a wave whose live lanes all hold camera rays tests them against the scene
    // bound (PathScene::bound_lo / _hi) and skips the query when none meets it (path_body).  The result
    // is the same either way; RTCORE_SCENE_BOUND=0 turns the skip off (same-call A/B, identity tests).
    // Kernel ms, one call, three rounds: C2 16.01-16.05 -> 14.97-15.00.
    p.scene_bound = 1;
    if (const char* e = getenv("RTCORE_SCENE_BOUND")) p.scene_bound = atoi(e) != 0 ? 1 : 0;
    // First bounce (rt_kernels.h, kFirstBounce / kFirstMasks; path_body): a wave of camera rays of one 8x8
    // block runs its query over the units the block can see.  The result is the same either way;
    // RTCORE_FIRST_BOUNCE=0 turns it off (run_path then sets no kFirstMasks), read per launch.
    bool first_bounce = true;
    if (const char* e = getenv("RTCORE_FIRST_BOUNCE")) first_bounce = atoi(e) != 0;
    if (first_bounce) p.scene_bound |= kFirstBounce;
    // Brute-force tile kernels: sample rounds (refill; ticket_rounds in rt_kernels.h has the rule).  The
    // result is the same either way: only when a lane starts its next sample changes.
    // RTCORE_SAMPLE_ROUNDS=0 turns them off, 2 runs every ticket in rounds, 1 (the default) lets each
    // wave choose per ticket; read per launch, like RTCORE_SCENE_BOUND.
    p.sample_rounds = 1;
    if (const char* e = getenv("RTCORE_SAMPLE_ROUNDS")) p.sample_rounds = std::max(0, std::min(2, atoi(e)));
    // BVH kernels: the shading phase runs once 28 lanes wait; a leaf step once 12 lanes are blocked
    // on a pending leaf.  Round 5, C4 with the walls as outer records (profiles/r05/c4_outer_sweep.log):
    // refill 24 / 28 / 32 at spec 16: 44.0 / 43.6 / 43.6 ms; spec 12 / 16 / 20 at refill 24: 43.8 /
    // 44.0 / 44.5; refill 28 + spec 12 (+ leaves of <= 2): 43.2 (43.0).  Earlier tree (round 2):
    // refill 8 / 16 / 20 / 24 / 28 / 32: 71.8 / 64.3 / 63.2 / 62.1-62.6 / 62.9 / 63.6 ms.
    p.refill = 28;
    if (const char* e = getenv("RTCORE_BVH_REFILL")) p.refill = std::max(1, std::min(64, atoi(e)));
    p.spec = 12;
    if (const char* e = getenv("RTCORE_BVH_SPEC")) p.spec = std::max(1, std::min(64, atoi(e)));
    // XCD-local item ranges: the 8x8 blocks cut into kMaxSplit runs of consecutive blocks (horizontal
    // strips of the tile), each dealt first to the workgroups of one XCD, so that one XCD's waves work
    // on neighbouring pixels and their closest-hit queries share that XCD's L2.  A single range hands
    // the whole frame out in order to all XCDs at once: every L2 then holds the nodes of the same
    // band.  RTCORE_XCD_SPLIT=0 turns it off (A/B).
    set_blocks(p, p.n_pad / 64);
    p.seed = seed;
    p.seed_key = rt_rng_seed_key(seed);
    p.sample_base = base;
    return p;
}

// rt_render_rays: a list of n rays planned as the tile 8 pixels wide and ceil(n / 8) tall, so that
// the item space is linear in the ray index: blocks_x = 1, block b's 64 pixels are the rays 64 b ..
// 64 b + 63 (ray = py * 8 + px), and the dispensers, the XCD ranges (runs of consecutive rays) and
// the partial layout are the tile's.  The RAYS kernels decode an item without the tile (item_ray)
// and bound it by n_rays.  The samples per item are those of a 1080p frame at this spp whatever n
// is (chunk_npix), so that a ray's fp32 partial sums, and with them its result, do not depend on
// how many rays share its call or on the host entry's chunking.
PathParams make_params_rays(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, uint64_t stream_base)
{
    PathParams p = make_params_for(kernel, 0, 0, 0, 0, 8, (int)((n + 7) / 8), spp, seed, base, 2073600.0);
    p.n_rays = (unsigned)n;
    p.stream_base = stream_base;
    return p;
}

// rt_render_pixels: a list of n frame pixels, planned as a ray list is: the 8-wide tile, so that entry
// i is pixel i & 63 of block i >> 6 and 64 consecutive entries share a wave, and the chunks of a
// 1080p frame at this spp whatever n is.  The samples per item are then min(64, ceil(spp / B)), B = 24
// for the brute-force kernels and 64 for the BVH kernel: a function of spp alone, so a pixel's fp32
// partial sums do not depend on the list it came in, and they are those of rt_render_device wherever
// that launch has the same samples per item.
PathParams make_params_pixels(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, int width, int height)
{
    PathParams p = make_params_for(kernel, 0, 0, 0, 0, 8, (int)((n + 7) / 8), spp, seed, base, 2073600.0);
    p.n_rays = (unsigned)n;
    p.n_frame_px = (unsigned)((uint64_t)width * (uint64_t)height);
    p.inv_frame_w = 1.0f / (float)width;
    return p;
}

// Most rays of one RAYS launch at this spp: 32-bit item indices, n_chunks slots per ray padded to
// whole blocks of 64, below the bound run_path holds every launch to (0xF0000000 items), and below
// 2^30 rays (n_pad is an int).  0 when not even one block fits.
int64_t render_rays_max_n(int kernel, int spp)
{
    const PathParams p = make_params_for(kernel, 0, 0, 0, 0, 8, 8, spp, 0, 0, 2073600.0);
    const int64_t blocks = (int64_t)(0xF0000000ull / ((uint64_t)p.n_chunks * 64u));
    return std::min<int64_t>(blocks * 64, (int64_t)1 << 30);
}

// rt_render_probes: make_params_rays with chunks_over = spp, which gives chunk = ceil(spp / spp) = 1 and
// `used` = spp real chunks of n_chunks = the next power of two; set_item_order deals no slot past them and,
// with no short chunk, every ticket is full-length but a block's last.  The tuned chunk counts and
// RTCORE_PATH_CHUNKS do not apply: what a probe's sample is must not depend on them.
PathParams make_params_probes(int kernel, int64_t n, int spp, uint64_t seed, uint64_t base, uint64_t stream_base)
{
    PathParams p = make_params_for(kernel, spp, 0, 0, 0, 8, (int)((n + 7) / 8), spp, seed, base, 2073600.0);
    p.n_rays = (unsigned)n;
    p.stream_base = stream_base;
    return p;
}

int64_t probes_max_n(int spp)
{
    const uint64_t items = 1ull << 26; // chunk_pipeline's figure (kChunkItems)
    uint64_t slots = 1;
    while (slots < (uint64_t)spp) slots *= 2; // (spp < 2^31: no overflow)
    return slots > items / 64 ? 0 : (int64_t)(items / slots); // a power of two >= 64: whole blocks
}

// Start rows: a wave that opens items builds every camera ray of those items with all its lanes and
// keeps them in a row buffer of its own; the sample start, which the lanes reach one by one, loads
// the lane's row instead of building the ray (refill).  For the brute-force tile launches that are
// not instrumented, of scenes without vertex-normal triangles (those instances spill already and
// would spill more), with a frustum camera without depth of field (another camera draws more per
// start and would need two rows per sample).  Up to kStartRowsMaxChunk samples per item: the loop at
// the item open runs `chunk` times for every lane, and a lane that opens an item alone pays it alone.
// The buffer is one row set per wave of the persistent grid; over kStartRowsCap the launch does
// without.  RTCORE_START_ROWS=0 turns them off; read per launch, like RTCORE_SCENE_BOUND.
StartRowsPlan plan_start_rows(int kernel, bool instrumented, bool vertex_normals, int camera_kind, bool dof, int chunk,
                              int grid_blocks)
{
    const StartRowsPlan off{false, 0, 0};
    if (kernel < 0 || kernel >= 2 || instrumented || vertex_normals || camera_kind != RT_CAMERA_FRUSTUM || dof) return off;
    if (chunk < 1 || chunk > kStartRowsMaxChunk || grid_blocks < 1) return off;
    if (const char* e = getenv("RTCORE_START_ROWS"))
        if (atoi(e) == 0) return off;
    const size_t bytes = (size_t)grid_blocks * 4u * (size_t)chunk * 64u * 16u;
    if (bytes > kStartRowsCap) return off;
    return StartRowsPlan{true, chunk, bytes};
}

// Launch overlap: which launches run beside their predecessor's tail, and what such a launch waits for
// before it rewrites what the other set's kernel reads (launch_params.h).
bool launch_overlaps(bool device_entry, bool repeats, bool bvh, bool instrumented, bool tracing, size_t partial_bytes)
{
    if (!device_entry || !repeats || bvh || instrumented || tracing || partial_bytes > kOverlapSetCap) return false;
    if (const char* e = getenv("RTCORE_LAUNCH_OVERLAP"))
        if (atoi(e) == 0) return false;
    return true;
}

OverlapWait overlap_wait(const OverlapChange& c)
{
    if (c.cull_replaced || c.jit_rebuilt || c.buffer_grown) return kOverlapHostWait; // memory is freed
    if (c.pkeys_rebuilt || c.cull_fresh) return kOverlapStreamWait;
    return kOverlapNoWait;
}

// Band-set launch: tile row r is frame row ((r / band) * stride + offset) * band + r % band; the
// kernel divides by a shift for power-of-two bands, else by the fp32 reciprocal.
void set_band(PathParams& p, int band, int stride, int offset)
{
    p.band = band;
    p.band_stride = stride;
    p.band_offset = offset;
    p.band_log2 = -1;
    for (int k = 0; k < 31; k++)
        if (band == (1 << k)) p.band_log2 = k;
    p.inv_band = 1.0f / (float)band;
}

int band_set_rows(int H, int band, int stride, int offset)
{
    int rows = 0;
    for (int b = offset; b * band < H; b += stride) rows += std::min(band, H - b * band);
    return rows;
}

// Largest band set of the split: the plane stride of a gather slot.
int band_slot_rows(int H, int band, int stride)
{
    int m = 0;
    for (int o = 0; o < stride; o++) m = std::max(m, band_set_rows(H, band, stride, o));
    return m;
}

// Adds one band set's planar accumulators (device layout, planes `plane` apart) into frame buffers
// in the C# [x, y] order (x * H + y).
void scatter_band_set(const unsigned char* slot, size_t plane, int W, int H, int band, int stride, int offset,
                      rt_color* sum_rgb, uint32_t* samples, uint32_t* misses)
{
    const double* hs = reinterpret_cast<const double*>(slot);
    const uint32_t* hn = reinterpret_cast<const uint32_t*>(hs + 3 * plane);
    const uint32_t* hm = hn + plane;
    parallel_ranges((size_t)W, 64, [&](size_t xa, size_t xb) { // column ranges: disjoint output spans
        int tr = 0;
        for (int b = offset; b * band < H; b += stride)
            for (int y = b * band; y < std::min(H, (b + 1) * band); y++, tr++)
                for (size_t x = xa; x < xb; x++) {
                    const size_t i = (size_t)tr * W + x, o = x * H + y;
                    sum_rgb[o].r += hs[i];
                    sum_rgb[o].g += hs[plane + i];
                    sum_rgb[o].b += hs[2 * plane + i];
                    samples[o] += hn[i];
                    misses[o] += hm[i];
                }
    });
}

int64_t list_tickets(const PathParams& p, uint32_t* out, int64_t cap_words)
{
    int64_t n = 0;
    for (int g = 0; g < p.n_split; g++)
        for (unsigned t = 0; t < p.split_tickets[g]; t++, n++) {
            unsigned first = 0, len = 0;
            ticket_items(p, (unsigned)g, t, first, len);
            if (3 * (n + 1) <= cap_words) {
                out[3 * n] = (uint32_t)g;
                out[3 * n + 1] = first;
                out[3 * n + 2] = len;
            }
        }
    return n;
}

} // namespace rtc
