/*
 * rtcore.h -- C ABI of the MI355X (gfx950) path-tracing core: the drop-in for
 * RaytracerCore's render worker.
 *
 * Reference seam (all paths relative to the reference repository):
 *   FullRaytracer constructs `Raytracer(this, Scene)` workers
 *   (RaytracerCore/Raytracing/FullRaytracer.cs:297-302).  Each worker loops
 *   GetWorkingTile() (FullRaytracer.cs:219-229) -> one sample per pixel of the tile
 *   into DoubleColor[tile.Width, tile.Height] with DoubleColor.Placeholder marking a
 *   primary miss (Raytracer.cs:294-330) -> OnTileFinished(tile, samples, elapsed)
 *   (FullRaytracer.cs:210-214).  The library replaces the body of that loop; the C#
 *   host keeps Scene / SceneLoader / Camera / SampleSet and calls this ABI through
 *   P/Invoke.
 *
 * Conventions
 *   - extern "C", cdecl, blittable structs only; every function returns RT_OK (0) or
 *     a negative rt_status; details via rt_last_error() (thread-local).
 *   - Host tile buffers use the C# rectangular-array order of DoubleColor[w, h]:
 *     element (x, y) of a w*h tile lives at offset x*h + y (y fastest),
 *     as in Raytracer.cs:305,317 and FullRaytracer.cs:328-339.
 *   - The library owns scene handles and device memory; callers own every output
 *     buffer and nothing is retained after a call returns.
 *   - A scene handle is bound to one device and is not re-entrant: calls on one handle
 *     are serialised by the caller.  Device-side calls may be queued on any stream; the
 *     library orders an operation on a stream other than the previous one after it
 *     (the launches share per-scene scratch), and any number of launches may be queued
 *     without a synchronisation.
 */
#ifndef RTCORE_H
#define RTCORE_H

#ifndef __HIPCC_RTC__
#include <stdint.h>
#include <stddef.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RTCORE_ABI_VERSION 6 /* 2: rt_frame_*, rt_render_bands, sample_base in rt_render_frame_multi;
                                3: rt_set_jit, rt_scene_get_jit_error, build stats [15..17];
                                4: rt_kernel_times;
                                5: rt_frame_submit / rt_frame_collect / rt_frame_inject_fault;
                                6: rt_trace_paths, rt_debug_ray, rt_bounce_type; rt_query_rays, rt_query_rays_device
                                   and rt_camera_rays were added under version 6 (purely additive): a host
                                   detects them by symbol; so were rt_select_pixels, rt_select_pixels_device,
                                   rt_select_rays, rt_select_rays_device and rt_debug_select_rays, and
                                   rt_render_rays and rt_render_rays_device, and rt_occluded_rays and
                                   rt_occluded_rays_device, and rt_render_pixels, rt_render_pixels_device,
                                   rt_adaptive_select_device and rt_debug_adaptive_select, and
                                   rt_primary_hits_device, rt_denoise_device and rt_debug_denoise, and
                                   rt_reproject_device and rt_debug_reproject, and rt_beam, rt_render_beams,
                                   rt_render_beams_device, rt_debug_beam_rays and rt_camera_beams, and
                                   rt_surfel, rt_gather_mode, rt_render_surfels, rt_render_surfels_device and
                                   rt_debug_surfel_rays_device, and rt_list_kind, rt_render_list and
                                   rt_render_list_device, and rt_occluded_surfels and
                                   rt_occluded_surfels_device, and rt_probe_sh, rt_render_probes,
                                   rt_render_probes_device, rt_debug_sh_basis and rt_debug_probe_fold, and
                                   rt_probe_grid, rt_probe_radiance_device, rt_debug_probe_radiance,
                                   rt_shade_probes, rt_shade_probes_device, rt_debug_probe_segments,
                                   rt_debug_probe_segments_device and rt_debug_shade_probes, and
                                   rt_probe_moments, rt_probe_select_params, rt_render_probe_list_device,
                                   rt_probe_select_device, rt_debug_probe_moments, rt_debug_probe_select and
                                   rt_debug_probe_error, and rt_obscurance, rt_obscurance_surfels_device,
                                   rt_obscurance_select_device, rt_debug_obscurance_fold,
                                   rt_debug_obscurance_select and rt_debug_obscurance_error, and
                                   rt_probe_relocate_params, rt_probe_relocation, rt_probe_positions_device,
                                   rt_debug_probe_positions, rt_relocate_probes_device, rt_debug_probe_relocate,
                                   rt_shade_probes_placed, rt_shade_probes_placed_device,
                                   rt_debug_probe_segments_placed, rt_debug_probe_segments_placed_device,
                                   rt_debug_shade_probes_placed, rt_shade_probes_depth_placed_device and
                                   rt_debug_shade_probes_depth_placed */

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_ARG = -1,      /* bad argument (null pointer, bad size, unknown kind)      */
    RT_ERR_HIP = -2,      /* a HIP runtime call failed                               */
    RT_ERR_OOM = -3,      /* device or host allocation failed                         */
    RT_ERR_NCCL = -4,     /* an RCCL call failed                                      */
    RT_ERR_PARSE = -5,    /* scene text could not be parsed (SceneLoader.cs:417-422) */
    RT_ERR_NODEVICE = -6, /* no HIP device available                                  */
    RT_ERR_STATE = -7     /* call out of order (e.g. render before a camera is set)   */
} rt_status;

/* Vec4D (RaytracerCore/Vectors/Vec4D.cs:16-91): 4 x fp64, 32 B, w=1 points, w=0 directions. */
typedef struct rt_vec4d { double x, y, z, w; } rt_vec4d;

/* DoubleColor (RaytracerCore/DoubleColor.cs:8-45): 3 x fp64, 24 B.  Placeholder = (-1,-1,-1). */
typedef struct rt_color { double r, g, b; } rt_color;

typedef enum rt_prim_kind {
    RT_PRIM_TRIANGLE = 0, /* Primitives/Triangle.cs */
    RT_PRIM_SPHERE = 1,   /* Primitives/Sphere.cs   */
    RT_PRIM_PLANE = 2     /* Primitives/Plane.cs    */
} rt_prim_kind;

typedef enum rt_prim_flags {
    RT_FLAG_MIRROR = 1,      /* Triangle.Mirror: parallelogram, u,v in [0,1]^2 (Triangle.cs:13-20)    */
    RT_FLAG_TWOSIDED = 2,    /* Primitive.TwoSided (Primitive.cs:78)                                   */
    RT_FLAG_INVERT = 4,      /* Primitive.Invert: flips Hit.Inside only (Primitive.cs:60-61)           */
    RT_FLAG_HASNORMALS = 8,  /* Triangle.HasNormals: per-vertex normals (Triangle.cs:45-52,209-219)   */
    RT_FLAG_TRANSFORMED = 16 /* Sphere.Transformed: ellipsoid via matrices (Sphere.cs:29-37)           */
} rt_prim_flags;

/*
 * One primitive as the C# Scene holds it after SceneLoader finalisation
 * (SceneLoader.cs:388-413), i.e. after Primitive.Transform.  Derived data
 * (triangle edges / face normal, bounding boxes, BVH) is computed by the library
 * with the reference's arithmetic.
 *   triangle: p[0..2] = Vert0..2.Position (world), n[0..2] = Vert0..2.Normal
 *   sphere:   p[0] = Center (object space), radius = Radius,
 *             to_obj = MatrixToObject, to_world = MatrixToWorld, to_normal = MatrixToNormal
 *             (row-major D00..D33; only read when RT_FLAG_TRANSFORMED is set)
 *   plane:    p[0] = Normal (unit, w=0), radius = OriginDistance
 * Materials are the raw backing fields; the library applies the Shininess<=0 gating of
 * the Specular / Refraction getters (Primitive.cs:111-129).
 */
typedef struct rt_prim {
    int32_t kind;
    int32_t flags;
    rt_vec4d p[3];
    rt_vec4d n[3];
    double radius;
    double to_obj[16];
    double to_world[16];
    double to_normal[16];
    rt_color emission, diffuse, specular, refraction;
    double shininess;
    double refractive_index;
} rt_prim;

typedef enum rt_camera_kind {
    RT_CAMERA_FRUSTUM = 0, /* Cameras/FrustumCamera.cs */
    RT_CAMERA_ORTHO = 1    /* Cameras/OrthoCamera.cs   */
} rt_camera_kind;

/*
 * The public fields of Camera (Cameras/Camera.cs:10-27) before InitRender.  The library
 * runs InitRender(width, height) itself (Camera.cs:54-63, FrustumCamera.cs:24-31,
 * OrthoCamera.cs:22-31) with the reference's arithmetic.
 */
typedef struct rt_camera {
    int32_t kind;
    int32_t reserved;
    rt_vec4d position, look_at, up;
    double fov_y;     /* FrustumCamera.fovY, radians                   */
    double size_mult; /* OrthoCamera.sizeMult                          */
    double image_plane, dof_amount, focal_length;
} rt_camera;

/* Scene-wide fields read on the hot path (Scene.cs:16-35). */
typedef struct rt_scene_params {
    int32_t width, height; /* Scene.Width / Height: the whole frame                        */
    int32_t recursion;     /* Scene.Recursion (default 3)                                  */
    int32_t debug_geom;    /* Scene.DebugGeom                                              */
    double air_ior;        /* Scene.AirRefractiveIndex (default 1.000293)                  */
    rt_color ambient;      /* Scene.AmbientRGB; (-1,-1,-1) = "ambient miss"                */
} rt_scene_params;

typedef struct rt_scene rt_scene; /* opaque */

/* Traversal strategy of the path-tracing kernel. */
typedef enum rt_traversal {
    RT_TRAVERSAL_AUTO = 0,  /* small scenes: brute force, grouped where a cost model
                               favours it; large scenes: the wide BVH                  */
    RT_TRAVERSAL_BRUTE = 1, /* every primitive, scene read through the scalar cache   */
    RT_TRAVERSAL_BVH = 2,   /* 4-wide quantised BVH (binned SAH, collapsed), LDS stack */
    RT_TRAVERSAL_BVH2 = 3,  /* the binary binned-SAH BVH it is collapsed from          */
    RT_TRAVERSAL_GROUPED = 4 /* brute force over groups of <= 8 primitives, a group
                                skipped when no ray of the wave meets its box          */
} rt_traversal;

typedef struct rt_scene_info {
    int32_t n_prims;
    int32_t ref_bvh_nodes;   /* nodes of the reference agglomerative BVH (BVH.cs:193-236); 0 until
                                the first exact debug pass builds it                         */
    int32_t ref_bvh_depth;
    int32_t sah_bvh_nodes;   /* nodes of the kernel's BVH2                                */
    int32_t sah_bvh_depth;
    int32_t traversal;       /* resolved rt_traversal of the path kernel                  */
    int32_t device;
    int32_t bvh_builder;     /* rt_bvh_builder that built the kernel's BVHs               */
    uint64_t device_bytes;   /* scene bytes resident in HBM                               */
} rt_scene_info;

/* Who builds the path kernel's BVH2 and its wide collapse at rt_scene_create. */
typedef enum rt_bvh_builder {
    RT_BVH_BUILDER_AUTO = 0, /* the GPU from 2^22 BVH primitives on, the host below
                                (RTCORE_BVH_BUILDER=host|gpu overrides AUTO)          */
    RT_BVH_BUILDER_HOST = 1, /* binned SAH on the host, collapsed to 4-wide            */
    RT_BVH_BUILDER_GPU = 2   /* PLOC on the device (Morton order, nearest-neighbour
                                merges by merged-box area), collapsed on the device   */
} rt_bvh_builder;

/* rt_scene_get_build_stats: [0] host preparation ms, [1] BVH build ms (wall, either
   builder), [2] upload ms, [3] GPU builder device ms, [4] PLOC rounds, [5] wide nodes,
   [6] wide-tree stack need; flat brute-force layout: [7] single world rectangles,
   [8] world boxes, [9] frames, [10] frame boxes, [11] rectangles tested one by one in
   frames, [12] other triangles, [13] spheres, [14] hot wide nodes staged in LDS;
   scene-specialised kernel of the last brute-force launch (rt_set_jit): [15] status (1 in use,
   0 not used, -1 build failed: see rt_scene_get_jit_error), [16] its hiprtc compile ms (0 when
   it came from the cache), [17] 1 if it came from the in-process or on-disk cache,
   [18] primitives per group of the grouped brute-force order (fixed at creation: 8 when the
   scene-specialised build was on then, else 4); [19] leaves of the wide tree, [20] of them compact
   (primitives of one kind and one set of test flags, read as 48-B records); [21] outer
   primitives: axis-aligned rectangles the BVH leaves out and tests as one group of rects and
   closed boxes when a query ends (host builder, scenes of more than 4096 BVH primitives) */
#define RT_BUILD_STATS_COUNT 22

/* ---------------------------------------------------------------- library ---- */
int rt_abi_version(void);
/* "src-sha256=<hex> extra=<flags>": the hash of the sources the library was built from and the
 * extra compiler flags of its build (raytracercore_amd/csrc/source_hash.py recomputes the hash). */
const char* rt_build_info(void);
int rt_device_count(void);
/* Copies the calling thread's last error message (NUL-terminated); returns its length. */
int rt_last_error(char* buf, int32_t cap);

/* ----------------------------------------------------------------- scenes ---- */
int rt_scene_create(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims,
                    int32_t device, rt_scene** out_scene);
int rt_scene_set_camera(rt_scene* scene, const rt_camera* camera);
/* RT_ERR_ARG (the scene's mode unchanged) for a mode the scene cannot run: brute force over more
   than 65535 triangles or 32767 spheres, a BVH deeper than the kernel's traversal stack. */
int rt_scene_set_traversal(rt_scene* scene, int32_t traversal);
int rt_scene_get_info(const rt_scene* scene, rt_scene_info* info);
void rt_scene_destroy(rt_scene* scene);
/* Process-wide builder choice for later rt_scene_create calls (default AUTO). */
int rt_set_bvh_builder(int32_t builder);
/* Copies min(n, RT_BUILD_STATS_COUNT) build statistics of the scene (see above). */
int rt_scene_get_build_stats(const rt_scene* scene, double* out, int32_t n);
/* Scene-specialised brute-force kernels (no reference counterpart: an MI355X code-generation
   choice).  With on = 1 (the default; the environment variable RTCORE_JIT=0 makes the default
   0) the brute-force traversals of scenes of <= 48 primitives launch a build of the path kernel
   whose primitive records are compile-time constants, made with hiprtc on the first launch per
   scene (and per camera for the grouped order) and cached in-process and on disk
   (RTCORE_JIT_CACHE, else $HOME/.cache/rtcore_jit).  Same arithmetic and results as the generic
   kernel, which runs when on = 0 or a build fails.  Process-wide; applies to later launches. */
int rt_set_jit(int32_t on);
/* The reason the last scene-specialised build of this scene failed ("" if none). */
int rt_scene_get_jit_error(const rt_scene* scene, char* buf, int32_t cap);
/* Host only (no device needed): compiles the embedded kernel sources for `arch` (e.g. "gfx950")
   as a scene-specialised build of an empty scene; returns the code object size, or a negative
   rt_status with the compiler log in `log` (may be NULL). */
int rt_debug_jit_compile(const char* arch, int32_t grouped, char* log, int32_t cap);
/* Host only (no device needed): the generated header of the scene-specialised build that
   rt_scene_create + rt_scene_set_camera would make for these primitives and camera (grouped = 0
   flat order, 1 grouped order; brute-force scenes of <= 48 primitives), for reading its code
   without a GPU (tools/jit_isa.py).  Returns the header length; copies it NUL-terminated into buf
   when cap exceeds the length. */
int rt_debug_jit_header(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims, const rt_camera* camera,
                        int32_t grouped, char* buf, int64_t cap);
/* Validation: checks the device-resident BVH2 and wide tree against the primitives (every
   child box contains the primitives below it, each primitive in exactly one leaf, depth and
   stack within what the kernels were sized for).  RT_ERR_STATE with the finding otherwise. */
int rt_scene_check_bvh(rt_scene* scene);
/* Host only (no device needed): the decomposition the brute-force kernels would test for these
   primitives -- out[0..9] = flat order: single world rectangles, world boxes (five or six faces of
   an axis-aligned box), frames (parallelograms along one affine frame's axes), frame boxes,
   rectangles tested one by one in frames, other triangles, spheres, planes; then the grouped
   order's group count and its slot count.  Copies min(n_out, 10) values. */
#define RT_LAYOUT_COUNT 10
int rt_debug_brute_layout(const rt_prim* prims, int32_t n_prims, int32_t* out, int32_t n_out);
/* Host only (no device needed): the order in which the path kernels' work dispensers deal the work
   items of a launch over a w x h tile at spp samples per pixel, computed by the function the kernels
   call.  chunks > 0: that many chunks per pixel (as RTCORE_PATH_CHUNKS), 0: the tuned count; pool
   > 0: items per ticket (a multiple of 64; above 64 the grouped kernel's defaults), 0: the flat
   kernel's; band > 0: the launch of the band set (band, band_stride, band_offset) of an h-row frame.
   A work item is ((block << log2(n_chunks)) + chunk) * 64 + pixel of the 8x8 block.  out gets three
   words per ticket -- item range, first item, items -- range by range, each range in the order its
   dispenser deals; tickets past cap_words / 3 are counted but not stored.  info (optional) gets
   {n_chunks, samples per chunk, items per full ticket, item ranges}.  Returns the number of
   tickets or a negative rt_status.  RTCORE_ITEM_ORDER=0 in the environment gives the order that
   also deals the empty chunk slots (A/B). */
int rt_debug_item_order(int32_t w, int32_t h, int32_t spp, int32_t chunks, int32_t pool, int32_t band,
                        int32_t band_stride, int32_t band_offset, uint32_t* out, int64_t cap_words, int32_t* info);
/* Host only (no device needed): how rt_render_pixels plans a list of n entries at spp samples per pixel
   for kernel 0 (BRUTE), 1 (GROUPED) or 3 (BVH): info[0..3] = {chunk slots per entry, samples per work
   item, work items per entry that hold samples, blocks of 64 entries}. */
int rt_debug_pixels_plan(int32_t kernel, int64_t n, int32_t spp, int32_t* info);
/* Host only (no device needed): the scene bound of these primitives -- the padded fp32 box over every
   primitive but the planes that the flat brute-force path kernel tests a wave of camera rays against, to
   skip the query of a wave that looks past the scene (RTCORE_SCENE_BOUND=0 turns the skip off).
   lo[3], hi[3]: the box; info (optional) gets {limit, pad}: origins with |x| + |y| + |z| above limit
   are not tested (they count as meeting the box), pad is what was added on every side.  Returns 0,
   1 when there is nothing to bound (an empty bound: no ray meets it), 2 when an extent is not finite
   (no skip for the scene), or a negative rt_status. */
int rt_debug_scene_bound(const rt_prim* prims, int32_t n_prims, float* lo, float* hi, float* info);
/* Host only (no device needed): the block cull of a brute-force launch -- which 8x8 pixel blocks of
   the launch's window hold no pixel whose camera rays can meet the scene bound of these primitives.
   The path kernels are not dealt such blocks: every sample of their pixels is a primary miss and one
   ray (RTCORE_BLOCK_CULL=0 turns the cull off, RTCORE_BLOCK_CULL_MIN=<blocks> sets the smallest launch
   that is culled).  width, height: the frame; (x0, y0, w, h): the window, tile pixel (px, py) being
   frame pixel (x0 + px, y0 + py), or with band > 0 the band set's frame row
   y0 + ((py / band) * band_stride + band_offset) * band + py % band (h = rt_band_rows of the set).
   dead gets one byte per block, row-major over ceil(w / 8) x ceil(h / 8) blocks (1 = dead), while
   they fit in cap; info (optional) gets {blocks per row, block rows}.  Every block is live when the
   proof is not available: a scene with planes, a bound without skip, a camera with depth of field or
   a value that is not finite, or one that stands inside or beside the bound.  Returns the number of
   live blocks or a negative rt_status. */
int rt_debug_block_cull(const rt_prim* prims, int32_t n_prims, const rt_camera* camera, int32_t width, int32_t height,
                        int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t band, int32_t band_stride,
                        int32_t band_offset, uint8_t* dead, int64_t cap, int32_t* info);
/* Host only (no device needed): the first bounce of a flat brute-force launch -- the test units of the
   flat order (each world rectangle, each world box, each frame with its rectangles and its box, each
   triangle record, each sphere record, in the order the kernel tests them) and, for every live 8x8 block
   of the window, a 64-bit mask whose bit u is clear when no camera ray of the block's pixels can meet
   unit u, by the block cull's own test and margins on the unit's padded box.  A wave whose live lanes
   all hold camera rays of one block tests those units alone; the results are the same bit for bit
   (RTCORE_FIRST_BOUNCE=0 turns it off).  The window and the band set as rt_debug_block_cull takes them.
   unit_first (optional, 65 entries) gets the first entry of each unit in unit_ids and the total after
   the last; unit_ids the primitive IDs the units stand for, while they fit in cap_ids; unit_box
   (optional, 6 floats per unit, 64 units) each unit's padded box, lo then hi; dead one byte per block
   and masks one word per live block, in the blocks' order, while they fit in cap_blocks; info
   (optional, 6 entries) {blocks per row, block rows, live blocks, 1 when the masks are in use, entries
   of unit_ids, the pad as float bits}.  The masks are all ones and not in use when the scene has
   planes, vertex-normal triangles, more than 64 units or no finite bound, or when the launch has no
   cull record: no block is dead (a camera inside the bound, depth of field).  Returns the number of
   units or a negative rt_status. */
int rt_debug_block_units(const rt_prim* prims, int32_t n_prims, const rt_camera* camera, int32_t width, int32_t height,
                         int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t band, int32_t band_stride,
                         int32_t band_offset, int32_t* unit_first, int32_t* unit_ids, int64_t cap_ids, float* unit_box,
                         uint8_t* dead, uint64_t* masks, int64_t cap_blocks, int32_t* info);
/* Host only (no device needed): the start rows of a brute-force launch -- a wave that opens work items
   builds every camera ray of those items with all its lanes and keeps them as 16-B rows in a buffer
   of its own, and a lane's sample start loads its row instead of building the ray; the results are
   the same bit for bit (RTCORE_START_ROWS=0 turns them off).  kernel 0 (BRUTE), 1 (GROUPED), 2 / 3
   (the BVH kernels: never); camera: its kind and depth of field decide; (w, h, spp): the launch, chunks
   > 0 that many chunks per pixel (as RTCORE_PATH_CHUNKS), 0 the tuned count; grid_blocks: blocks of
   256 threads of the persistent grid; flags: 1 an instrumented launch, 2 a scene with vertex-normal
   triangles (neither gets them).  info[0..2] = {rows per wave, bytes of the buffer, samples per work
   item}; rows and bytes are 0 when off.  Off for more than 16 samples per item and for a buffer over
   256 MiB.  Returns 1 (on), 0 (off) or a negative rt_status. */
int rt_debug_start_rows(int32_t kernel, const rt_camera* camera, int32_t w, int32_t h, int32_t spp, int32_t chunks,
                        int32_t grid_blocks, int32_t flags, int64_t* info);
/* Host only (no device needed): the two decisions of launch overlap.  Returns 1 when a
   launch runs on a launch set's own stream, beside the tail of the launch before it, 0 when it runs
   serially on the caller's stream, or a negative rt_status.  launch_flags: 1 the launch is
   rt_render_device's or rt_render_bands_device's (no other entry overlaps), 8 it repeats the width,
   height and samples of the launch before it through those entries (no other launch overlaps),
   16 it runs a BVH kernel (only the brute-force kernels overlap), 2 instrumented (rt_scene_set_stats), 4 tracing (rt_trace_paths); partial_bytes: the launch's partials, which a second
   set holds again (over 4 GiB: serial); RTCORE_LAUNCH_OVERLAP=0, read per launch, turns it off.  *wait
   gets what an overlapped launch waits for before it rewrites state the other set's path kernel may be
   reading, from change_flags: 1 the pixel keys are rebuilt (a new seed), 2 a fresh cull record is
   uploaded, 4 it replaces a cached one, 8 the scene-specialised kernel is rebuilt, 16 a work buffer
   grows -- 0 nothing, 1 the other set's path kernel on the set's stream, 2 the same on the host (memory
   is freed: flags 4, 8, 16). */
int rt_debug_launch_overlap(int32_t launch_flags, uint64_t partial_bytes, int32_t change_flags, int32_t* wait);
/* Measurement of a wavefront split's traversal stage.  rt_debug_ray_log: while
   the next instrumented launch of a BVH kernel runs (rt_scene_set_stats; one launch only, then
   logging is off again), the kernel appends every finished query
   to d_log as 3 float4 (origin, previous primitive ID | direction, frame pixel index | closest t,
   hit slot, bounce) at the
   device counter *d_count, up to cap records (d_log = NULL turns logging off).
   rt_debug_trace_rays: the trace-only kernel (wide BVH, no shading) over n logged queries on
   `stream`, with waves_per_simd 6, 7 or 8; writes (t, slot) per query to d_hits, optional
   counters to d_stats[3] (node-step lane slots, leaf-step lane slots, lane slots in all) and the
   kernel's time (hipEvents) to *ms.  BVH traversal modes of a scene without planes only. */
int rt_debug_ray_log(rt_scene* scene, void* d_log, uint32_t cap, void* d_count);
/* Host only: the kernels' vertex-normal re-hit test -- Triangle.RayTraceAVXFaster in
   fp64 on the ray that leaves the triangle (v0, e01, e02) from its point fma(e01, u, fma(e02, v, v0))
   along dir (fp32, as the kernel holds it).  Returns 1 if that query meets the triangle again, 0 if
   not (negative rt_status on bad arguments); *inside = its Inside flag, *t its distance, origin[3]
   the start point used. */
int rt_debug_vn_rehit(const double* v0, const double* e01, const double* e02, int32_t mirror, double u, double v,
                      const float* dir, int32_t* inside, double* t, double* origin);
int rt_debug_trace_rays(rt_scene* scene, const void* d_rays, uint32_t n, void* d_hits, int32_t waves_per_simd,
                        void* d_stats, void* stream, float* ms);

/* ------------------------------------------------------- host-buffer renders --- */
/*
 * Accumulate spp samples (sample indices sample_base .. sample_base+spp-1) for every
 * pixel of the tile [x0, x0+w) x [y0, y0+h) into caller buffers laid out x*h + y:
 *   sum_rgb[i] += sum of non-miss sample colours   (SampleSet.AddSample, SampleSet.cs:32-36)
 *   samples[i] += non-miss samples, misses[i] += misses (SampleSet.AddMiss, :41-44)
 * rays_out (may be NULL) receives the number of Scene.RayTrace-equivalents (Mrays unit).
 */
int rt_render_tile(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp,
                   uint64_t seed, uint64_t sample_base, rt_color* sum_rgb, uint32_t* samples,
                   uint32_t* misses, uint64_t* rays_out);

/*
 * Exactly Raytracer.Render's one-pass contract (Raytracer.cs:305-320): one sample per
 * pixel (index sample_index), written (not accumulated) to out[x*h + y];
 * primary misses are DoubleColor.Placeholder (-1,-1,-1).
 */
int rt_render_tile_1spp(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h,
                        uint64_t seed, uint64_t sample_index, rt_color* out);

/*
 * DebugRaycaster Primitives mode (DebugRaycaster.cs:193-199,241): integer-pixel primary
 * ray, no jitter / DOF, closest hit by the reference's BVH query in fp64
 * (Scene.cs:65-111).  ids_out[x*h + y] = Primitive.ID (insertion order) or -1 on a miss.
 */
int rt_primary_ids(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* ids_out);

/*
 * DebugRaycaster BoundingVolumes mode (DebugRaycaster.cs:200-212): for the same integer-pixel
 * primary rays, BVH<T>.GetIntersectionCount (BVH.cs:352-363) over the reference BVH in fp64 --
 * the number of nodes whose own box the ray meets (Volume.Intersect(ray).far >= 0), descending
 * only through those.  counts_out[x*h + y]; 0 where the root is missed.
 */
int rt_bvh_counts(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t* counts_out);

/* ------------------------------------------------------------ path inspection --- */
/* Raytracer.BounceType (Raytracer.cs:14-26), same values. */
typedef enum rt_bounce_type {
    RT_BOUNCE_SKIPPED = 0,            /* no record (past the end of the path)                  */
    RT_BOUNCE_DIFFUSE = 1,
    RT_BOUNCE_SPECULAR = 2,
    RT_BOUNCE_SPECULAR_FAIL = 3,      /* a specular direction into the surface ends the path   */
    RT_BOUNCE_TRANSMITTED = 4,
    RT_BOUNCE_EMISSION = 5,           /* no event chosen: the path ends on the emission        */
    RT_BOUNCE_PURE_BLACK = 6,         /* a primitive of no luminance at all                    */
    RT_BOUNCE_RECURSION_COMPLETE = 7, /* the hit at bounce index Scene.Recursion               */
    RT_BOUNCE_MISSED = 8,
    RT_BOUNCE_DEBUG = 9               /* Scene.DebugGeom                                       */
} rt_bounce_type;

/*
 * Raytracer.DebugRay (Raytracer.cs:28-33) with its Hit, one per bounce: 96 B, six 16-byte rows,
 * no pointers.  The floats are the kernel's own fp32 values, not widened.
 *   offset  0  prim_id       Primitive.ID (insertion order), -1 on a miss
 *           4  type          rt_bounce_type
 *           8  inside        Hit.Inside after Primitive.Invert (0 / 1; 0 on a miss)
 *          12  distance      Hit.Distance along `direction` (0 on a miss, and on the re-hit of a
 *                            vertex-normal triangle the ray leaves)
 *          16  fresnel       DebugRay.FresnelRatio: NaN where GetColor does not reach the Fresnel block
 *                            (Raytracer.cs:120), exactly 1 on total internal reflection (:144)
 *          20  cos_in        the `cos` of Raytracer.cs:115, -roughNormal . direction; NaN on the types
 *                            MISSED, DEBUG and RECURSION_COMPLETE, which end before it
 *          24  bounce        the record's index in its path, 0 = the camera ray
 *          28  reserved0     0
 *          32  position[3]   Hit.Position as the shading uses it (0 on a miss)
 *          44  normal[3]     Hit.Normal, facing the incoming ray (0 on a miss; NaN inside a
 *                            vertex-normal triangle, Triangle.GetNormal's quirk)
 *          56  origin[3]     the ray traced at this bounce
 *          68  direction[3]
 *          80  tint[3]       the path's tint before this bounce
 *          92  reserved1     0
 */
typedef struct rt_debug_ray {
    int32_t prim_id;
    int32_t type;
    int32_t inside;
    float distance;
    float fresnel;
    float cos_in;
    int32_t bounce;
    int32_t reserved0;
    float position[3];
    float normal[3];
    float origin[3];
    float direction[3];
    float tint[3];
    int32_t reserved1;
} rt_debug_ray;

/* Most records (w * h * spp * (Scene.Recursion + 1)) of one rt_trace_paths call: 96 MB of them. */
#define RT_TRACE_MAX_RECORDS (1 << 20)

/*
 * Raytracer.GetDebugTrace (Raytracer.cs:254-260, 289-292; RayInspector.RunTraces) for the
 * library's own samples: the samples sample_base .. sample_base+spp-1 of every pixel of the tile,
 * exactly as a render with this seed traces them (the same kernels in the scene's traversal mode;
 * always the generic ones, whatever rt_set_jit says), with one record per bounce.
 *   sample k of pixel (x, y) of the tile is s = (x*h + y)*spp + k
 *   rays_out[s*(recursion+1) + i]   bounce i of the sample; the records past n_rays_out[s] are all
 *                                   zero (type RT_BOUNCE_SKIPPED)
 *   n_rays_out[s]  (may be NULL)    records of the sample, 1 .. recursion+1
 *   colors_out[s]  (may be NULL)    the sample's value as rt_render_tile_1spp returns it for
 *                                   sample_index = sample_base + k, (-1,-1,-1) on a primary miss
 * RT_ERR_ARG, before anything is launched, for a null rays_out, spp <= 0, a tile outside the frame
 * or more than RT_TRACE_MAX_RECORDS records.  Synchronous, on the scene's own stream; the counters
 * of rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times and the scene-specialised
 * kernels are left as they were.
 */
int rt_trace_paths(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp,
                   uint64_t seed, uint64_t sample_base, rt_debug_ray* rays_out, int32_t* n_rays_out,
                   rt_color* colors_out);

/* ---------------------------------------------------------------- ray queries --- */
/* Ray (Vectors/Ray.cs): origin (w = 1) and an already-normalised direction (w = 0), taken as given. 64 B. */
typedef struct rt_ray { rt_vec4d origin, direction; } rt_ray;

/* Hit (Hit.cs) of Scene.RayTrace(ray, null): 48 B, three 16-byte rows, no pointers.
 *   0  prim_id      Primitive.ID (insertion order), -1 on a miss
 *   4  inside       Hit.Inside after Primitive.Invert (0 / 1; 0 on a miss)
 *   8  distance     Hit.Distance (0 on a miss); RT_QUERY_FAST: the kernel's fp32 value widened exactly
 *  16  position[3]  RT_QUERY_FAST: as rt_debug_ray.position; RT_QUERY_EXACT: 0
 *  28  normal[3]    RT_QUERY_FAST: as rt_debug_ray.normal (same NaN quirk); RT_QUERY_EXACT: 0
 *  40  reserved[2]  0 */
typedef struct rt_hit { int32_t prim_id, inside; double distance; float position[3], normal[3]; int32_t reserved[2]; } rt_hit;

typedef enum rt_query_mode {
    RT_QUERY_FAST = 0, /* the path kernels' own fp32 closest hit, in the scene's traversal mode (BRUTE, GROUPED
                          or BVH; RT_ERR_STATE on a BVH2 scene); the ray rounded to fp32 component by component */
    RT_QUERY_EXACT = 1 /* the fp64 reference query of rt_primary_ids (reference BVH, built on first use), in
                          every traversal mode: the reference's own answer bit for bit */
} rt_query_mode;

/*
 * Scene.RayTrace(ray, null) (Scene.cs:113-120) for rays the caller brings: hits_out[i] answers rays[i].
 * A ray with a non-finite component or a zero direction is a miss.  n == 0 returns RT_OK and touches
 * nothing; RT_ERR_ARG, before anything is launched, for a null pointer, n < 0 or an unknown mode.  The
 * generic kernels run, whatever rt_set_jit says; the counters of rt_scene_get_stats, an armed
 * rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels are left as they were.  No camera
 * is needed.  RT_QUERY_EXACT: RT_ERR_STATE from the host entry (prim_id -2 in the device entry's output)
 * where the reference BVH is deeper than the exact kernel's traversal stack, as rt_primary_ids.
 * rt_query_rays takes host buffers and is synchronous, on the scene's own stream: it works in chunks
 * of at most 2^19 rays (RTCORE_QUERY_CHUNK in the environment sets another size), two of them resident,
 * so its device scratch and its pinned staging stay at about 117 MB each for any n, and a chunk's
 * upload and the previous chunk's download overlap the kernel between them.
 * rt_query_rays_device takes device buffers and is asynchronous on `stream` (a hipStream_t, NULL = the
 * default stream), ordered like the device-resident renders.
 */
int rt_query_rays(rt_scene* scene, int32_t mode, const rt_ray* rays, int64_t n, rt_hit* hits_out);
int rt_query_rays_device(rt_scene* scene, int32_t mode, const rt_ray* d_rays, int64_t n, rt_hit* d_hits, void* stream);
/* Host only, no device: Camera.GetRay(x, y).Offset(imagePlane) (DebugRaycaster.cs:241) for the integer
   pixels of the tile [x0, x0+w) x [y0, y0+h) of a width x height frame, out[x*h + y]: the rays
   rt_primary_ids traces.  RT_ERR_ARG for a null pointer, an unknown camera kind, w or h <= 0 or a tile
   outside the frame. */
int rt_camera_rays(const rt_camera* camera, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w,
                   int32_t h, rt_ray* out);

/* ------------------------------------------------------------ occlusion queries --- */
/*
 * "Is anything between this point and that one": any-hit visibility for segments the caller brings.
 *   occluded_out[i] = 1  when Scene.RayTrace(rays[i], null) returns a hit with Hit.Distance < t_max[i]
 *                        (strictly, as RayTracePrimitives' own currentHit.Distance < hit.Distance,
 *                        Scene.cs:85-86), with the culling of Primitive.RayTrace (Primitive.cs:46-75) and
 *                        no skip hit: one-sided, two-sided and inverted primitives as in a render;
 *                     0  otherwise.
 * The segment starts at the ray's origin: there is no skip primitive and no t_min, and a caller that
 * leaves a surface offsets the origin itself.
 * t_max: NULL means +inf for every ray ("does this ray hit anything").  t_max[i] that is NaN, <= 0 or
 * (RT_QUERY_FAST) rounds to 0 in fp32 is an empty segment: the answer is 0.  +inf is valid.  A ray with a
 * non-finite component or a zero direction gives 0 (the rule of rt_query_rays).
 * RT_QUERY_FAST: the fp32 tests of the path kernels in the scene's traversal mode (BRUTE, GROUPED, or BVH
 *   with either builder; on a BVH2 scene RT_ERR_STATE with the message rt_query_rays gives), always the
 *   generic kernels, whatever rt_set_jit says.  The ray is rounded to fp32 as for rt_query_rays and
 *   t_max[i] to fp32 to nearest.  The traversal is not the closest-hit one: it is unordered, bounded by
 *   t_max and ends at the first accepted primitive.  Its answer is that of rt_query_rays(RT_QUERY_FAST)
 *   on the same ray in the same mode: a hit exists and its fp32 distance is < (float)t_max[i].  The two
 *   may differ only where that distance lies within the slack of the kernels' box culling of t_max: boxes
 *   (the grouped order's group boxes, the wide tree's children) are kept up to t_max * 1.00000024, the
 *   factor in the kernels' slab and wide_visit, and the closest-hit search culls by its shrinking best
 *   distance with the same factor, so a primitive within 2.4e-7 (relative) of the bound or of another hit
 *   can be tested by one search and not by the other.
 * RT_QUERY_EXACT: the fp64 reference query of rt_primary_ids in every traversal mode (reference BVH,
 *   built on first use): its Hit.Distance compared with t_max[i] in fp64, the reference's own answer.  On
 *   a traversal-stack overflow the device entry writes 255 for that ray and the host entry returns
 *   RT_ERR_STATE (rt_query_rays reports the same by prim_id -2).
 * n == 0 returns RT_OK and touches nothing; RT_ERR_ARG, before anything is launched, for a null scene,
 * rays or output pointer, n < 0 or an unknown mode.  The counters of rt_scene_get_stats, an armed
 * rt_debug_ray_log, the rt_kernel_times ring and the scene-specialised kernels are left as they were.  No
 * camera is needed.
 * rt_occluded_rays takes host buffers and is synchronous, on the scene's own stream; any n, in chunks of at
 * most 2^19 rays (RTCORE_QUERY_CHUNK sets another size), two of them resident with the overlap of
 * rt_query_rays; per ray it stages 72 B up (64 B when t_max is NULL) and 1 B down.
 * rt_occluded_rays_device takes device buffers and is asynchronous on `stream`, ordered like the
 * device-resident renders (the per-scene scratch rule of the preamble); launches are split at 2^30 rays.
 */
int rt_occluded_rays(rt_scene* scene, int32_t mode, const rt_ray* rays, const double* t_max, int64_t n,
                     uint8_t* occluded_out);
int rt_occluded_rays_device(rt_scene* scene, int32_t mode, const rt_ray* d_rays, const double* d_t_max, int64_t n,
                            uint8_t* d_occluded, void* stream);

/*
 * rt_occluded_surfels / rt_occluded_surfels_device: how many of a surface point's sample segments are
 * occluded.  rt_occluded_rays wants one rt_ray and one t_max per SAMPLE; here the caller brings one
 * rt_surfel (below, "radiance queries") and one t_max per POINT and the device draws the directions: ambient
 * occlusion, sky visibility, a probe's openness, from 64 B (+ 8 B of t_max) up and 4 B down per point for
 * any number of samples.
 * The sample (normative).  Sample k of entry e is the ray rt_render_surfels defines for sample k of record
 *   e: rt_rng_init(seed, stream_base + e, sample_base + k), U1 and U2 from its first two draws, the formulas
 *   of rt_surfel in gather_mode; the ray rt_debug_surfel_rays_device reports.  No further draw is used.  The
 *   stream is keyed by the entry number, not by the list position.
 * The segment starts at that ray's origin and ends at t_max[e], indexed by entry; NULL means +inf for every
 *   entry.  rt_occluded_rays' rules hold word for word: t_max[e] is rounded to fp32 to nearest; NaN, <= 0 or
 *   rounding to 0 is an empty segment (no sample occluded); +inf is valid.  There is no skip primitive and
 *   no t_min: the caller offsets the position.
 * Promise 1 (bit for bit): sample k of entry e counts as occluded exactly when
 *   rt_occluded_rays_device(RT_QUERY_FAST) answers 1 for that reported ray with t_max[e], on the same scene
 *   in the same traversal mode (BRUTE, GROUPED, or BVH with either builder): always the generic kernels,
 *   with the order of the records outside the main loop and RTCORE_OCCLUDED_EARLY as that entry reads them.
 * Accumulation: occluded[e] += the count and samples[e] += spp, both added to; samples may be NULL.  An
 *   invalid surfel (rt_render_surfels' definition) counts as spp unoccluded samples, rt_occluded_rays' rule
 *   that a bad ray gives 0.  Every listed entry below n_records therefore gets exactly samples += spp.
 * Promise 2: an entry's counts depend only on (seed, stream_base + e, the sample indices, the record,
 *   t_max[e], the traversal mode); not on n, on n_records, on the entry's place in the list, on the host
 *   entry's chunking or on the stream.  The counts are integers, so this holds however the kernels split the
 *   samples; two calls over sample ranges that join give the counts of one call over the joined range.
 * The list (device entry): d_index[j], j < n, names the entries; NULL is the identity and n must equal
 *   n_records.  An entry >= n_records is skipped and nothing is written for it; an entry named twice is
 *   undefined.  d_surfels, d_t_max, d_occluded and d_samples have n_records elements.  The host entry has no
 *   list: n surfels, surfel i keyed stream_base + i.
 * Errors, before anything is launched: RT_ERR_ARG for an unknown gather_mode (checked first), a null scene,
 *   n < 0, spp <= 0; then, for n > 0, a null surfels or occluded pointer, n_records <= 0 or >= 2^32, a null
 *   index with n != n_records.  RT_ERR_STATE on a BVH2 scene, with rt_query_rays' message.  n == 0 returns
 *   RT_OK and touches nothing.  No camera is needed.  The counters of rt_scene_get_stats, an armed
 *   rt_debug_ray_log, the rt_kernel_times ring and the scene-specialised kernels are left as they were.
 * rt_occluded_surfels_device is asynchronous on `stream`, ordered like the device-resident renders (the
 *   per-scene scratch rule of the preamble); it splits into as many launches as 2^30 (entry, sample) pairs
 *   per launch need.
 * rt_occluded_surfels takes host buffers and is synchronous, on the scene's own stream, for any n: in
 *   rt_occluded_rays' chunks (2^19 surfels, RTCORE_QUERY_CHUNK, two resident, the copies beside the kernels)
 *   and buffers.
 * Not part of it: RT_QUERY_EXACT (the answer is defined through the fp32 ray; the exact any-hit kernel stays
 *   a per-ray entry).  A falloff weight, the bent normal and a loop that adapts spp to the result exist under
 *   another name: rt_obscurance_surfels_device and rt_obscurance_select_device ("obscurance at surfels"), which
 *   pay for them with a closest-hit query; these counts remain the cheap path.
 */
struct rt_surfel; /* (defined under "radiance queries") */
int rt_occluded_surfels_device(rt_scene* scene, int32_t gather_mode, const struct rt_surfel* d_surfels, int64_t n_records,
                               const uint32_t* d_index, int64_t n, const double* d_t_max, int32_t spp, uint64_t seed,
                               uint64_t sample_base, uint64_t stream_base, uint32_t* d_occluded, uint32_t* d_samples,
                               void* stream);
int rt_occluded_surfels(rt_scene* scene, int32_t gather_mode, const struct rt_surfel* surfels, int64_t n,
                        const double* t_max, int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base,
                        uint32_t* occluded, uint32_t* samples);

/* ------------------------------------------------------------ selection pass --- */
/* DebugRaycaster's Selection mode (DebugRaycaster.cs:174-192): the overlay that shows only what
 * SceneInspector handed to SetDisplayOnly.  One ray per pixel (or per caller's ray) is tested against
 * every item of a list, in list order:
 *     dist = +inf; winner = none
 *     for each item: curD = item.Intersect(ray); if (curD <= dist) { dist = curD; winner = item }
 * so NaN never wins, the later of two items at equal distances wins, and +inf wins over "none".
 *   RT_SELECT_PRIM  PrimitiveIntersector: Primitive.RayTrace(ray, null) of primitive `index` (its
 *                   Primitive.ID, insertion order) with its two-sided / invert culling; Hit.Distance,
 *                   NaN on a miss.  No bounding box is tested first.
 *   RT_SELECT_NODE  BVHIntersector: AABB.IntersectAVX of the box of node `index` of the reference BVH
 *                   in depth-first pre-order (node, left subtree, right subtree: the index of its box
 *                   in rt_ref_bvh_export's `boxes`); near when near >= 0, else far (the origin inside
 *                   the box), NaN on a miss.  SkipVolume nodes are tested like every other.
 * All in fp64, in the reference's rounding order: the reference's own answer bit for bit. */
typedef enum rt_select_kind { RT_SELECT_PRIM = 0, RT_SELECT_NODE = 1 } rt_select_kind;
typedef struct rt_select_item { int32_t kind, index; } rt_select_item; /* 8 B */
/* 16 B, one 16-byte row:
 *   0  item      index in the caller's list of the winner, -1 when nothing won
 *   4  reserved  0
 *   8  distance  the winning curD (may be +inf), 0 when nothing won */
typedef struct rt_selection { int32_t item, reserved; double distance; } rt_selection;
/* Most item tests (w * h * n_items, or n * n_items) of one call. */
#define RT_SELECT_MAX_TESTS (1ull << 32)

/*
 * rt_select_pixels*: the rays of rt_primary_ids (Camera.GetRay(x, y).Offset(imagePlane) at the integer
 * pixels of the tile; a camera must be set).  Host output out[x*h + y], device output d_out[y*w + x].
 * rt_select_rays*: rays the caller brings, out[i] answers rays[i]; a ray with a non-finite component
 * or a zero direction gives item -1 (the rule of rt_query_rays).  No camera is needed.
 * `items` is always a host array of n_items records; the library copies it to the device.  n_items == 0
 * is valid (item -1 everywhere); n == 0 returns RT_OK and touches nothing.  RT_ERR_ARG, before anything
 * is launched, for a null pointer, n_items < 0, n < 0, an unknown kind, a primitive index outside
 * [0, n_prims), a node index outside the reference BVH, a tile outside the frame, or more than
 * RT_SELECT_MAX_TESTS item tests.  The reference BVH is built (on first use) only when a node item is
 * present.  The counters of rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times and the
 * scene-specialised kernels are left as they were.
 * The host-buffer entry points are synchronous, on the scene's own stream (rt_select_rays in chunks of
 * at most 2^19 rays); the _device ones take device buffers and are asynchronous on `stream` (a
 * hipStream_t, NULL = the default stream), ordered like the device-resident renders.
 */
int rt_select_pixels(rt_scene* scene, const rt_select_item* items, int32_t n_items, int32_t x0, int32_t y0, int32_t w,
                     int32_t h, rt_selection* out);
int rt_select_pixels_device(rt_scene* scene, const rt_select_item* items, int32_t n_items, int32_t x0, int32_t y0,
                            int32_t w, int32_t h, rt_selection* d_out, void* stream);
int rt_select_rays(rt_scene* scene, const rt_select_item* items, int32_t n_items, const rt_ray* rays, int64_t n,
                   rt_selection* out);
int rt_select_rays_device(rt_scene* scene, const rt_select_item* items, int32_t n_items, const rt_ray* d_rays, int64_t n,
                          rt_selection* d_out, void* stream);
/* Host only, no device: rt_select_rays for the scene these primitives make, by the same per-item
   functions and the same fold compiled for the CPU (the reference BVH is built when a node item asks
   for it).  RT_ERR_ARG as rt_select_rays, and for n_prims < 0 or an unknown primitive kind. */
int rt_debug_select_rays(const rt_prim* prims, int32_t n_prims, const rt_select_item* items, int32_t n_items,
                         const rt_ray* rays, int64_t n, rt_selection* out);

/* -------------------------------------------------- device-resident renders --- */
/*
 * The same work as rt_render_tile on device buffers (framebuffer stays in HBM).
 * Device layout is row-major over the tile, i = y*w + x, with planar accumulators:
 *   d_sum    : 3 * w*h doubles, planes R | G | B
 *   d_samples, d_misses : w*h uint32
 *   d_rays   : one uint64 counter (added to)
 * `stream` is a hipStream_t (NULL = default stream).  Asynchronous: returns after launch.
 */
int rt_render_device(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t spp,
                     uint64_t seed, uint64_t sample_base, double* d_sum, uint32_t* d_samples,
                     uint32_t* d_misses, unsigned long long* d_rays, void* stream);

/* ------------------------------------------------------------ radiance queries --- */
/*
 * Raytracer.GetColor(ray) (Raytracer.cs:248-252, the bounce loop of :65-246) for rays the caller
 * brings: spp path-traced samples of every ray, by the fp32 path kernels in the scene's traversal mode
 * (BRUTE, GROUPED or BVH with either builder; RT_ERR_STATE on a BVH2 scene, as RT_QUERY_FAST), always
 * the generic kernels, whatever rt_set_jit says.  A probe, a bake, or a camera the library does not
 * have (equirectangular, fisheye, a stereo pair, a lens model of the host's own).  No camera is needed.
 *
 * Accumulation is SampleSet's, exactly as rt_render_tile / rt_render_device define it, with "pixel"
 * replaced by "ray i"; everything is added to, not written:
 *   sum_rgb[i] += the colours of the samples of rays[i] that are not primary misses
 *   samples[i] += the count of those samples
 *   misses[i]  += the samples whose bounce 0 misses (DoubleColor.Placeholder, Raytracer.cs:86-87)
 *   rays_out / d_rays_count (may be NULL) += the Scene.RayTrace equivalents, in rt_render_tile's unit
 * Device layout: d_sum is three planes R | G | B of n doubles each; d_samples, d_misses n each.
 *
 * The ray follows rt_ray's contract: the direction is already normalised and is taken as given.  Origin
 * and direction are rounded to fp32 component by component (the rule of RT_QUERY_FAST) and traced as
 * bounce 0.  Nothing normalises them: Ray.Directional at i = 0 (Raytracer.cs:74-75) is the caller's job,
 * as the camera's ray is normalised once where it is made; the renormalisations of the rays that leave
 * bounces 2, 5, ... (traced as bounces 3, 6, ...) stay as they are.  A ray with a non-finite component
 * or a zero direction is a primary miss for all spp samples (the rule of rt_query_rays) and adds nothing
 * to the ray count.
 *
 * The random stream (normative): sample k of ray i draws from
 *     rt_rng_init(seed, stream_base + i, sample_base + k)      (rtcore_rng.h)
 * with the first two draws discarded -- the two GetCameraRay spends on subX and subY (Raytracer.cs:264-265),
 * which a caller's ray has no use for -- and the bounce draws following in rtcore_rng.h's order.  So
 *   - a ray's result depends only on (seed, stream_base + i, the sample indices, the ray) and on the
 *     scene's traversal mode: not on n, on the ray's position in the list, on the host entry's chunking
 *     or on the wave it lands in (the samples per work item are a function of spp alone);
 *   - for a camera without depth of field, the bounce-0 ray rt_trace_paths reports for sample k of frame
 *     pixel (x, y) (fp32 origin and direction of record 0), brought back with
 *     stream_base = y * frame_width + x, sample_base = k, spp = 1, gives that sample's colour bit for
 *     bit: a host can recompute, re-order or redistribute the library's own samples.
 * Coherence: rays 64 j .. 64 j + 63 of a call share a wave for every sample (work items are (sample
 * chunk, ray) pairs dealt in blocks of 64 consecutive rays), so list neighbouring rays next to each
 * other: the grouped order's wave-level box skip and the BVH kernel's memory locality depend on it.
 *
 * n == 0 returns RT_OK and touches nothing.  RT_ERR_ARG, before anything is launched, for a null scene,
 * rays, sum, samples or misses pointer, n < 0 or spp <= 0.  The counters of rt_scene_get_stats, an armed
 * rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels are left as they were.
 * rt_render_rays takes host buffers, is synchronous on the scene's own stream and accepts any n: it
 * works in chunks of at most 2^19 rays (RTCORE_QUERY_CHUNK in the environment sets another size, as for
 * rt_query_rays; fewer when spp is so large that a chunk's work items would pass 2^26), two of them
 * resident, so device scratch (1 GiB of partial sums at most, 96 MiB of rays and records) and pinned
 * staging (96 MiB) stay bounded, and a chunk's upload and the previous chunk's download overlap the
 * kernel between them.  RT_ERR_ARG when not even 64 rays fit (spp above about 2^26 samples).
 * rt_render_rays_device takes device buffers and is asynchronous on `stream` (a hipStream_t, NULL =
 * the default stream), ordered like the device-resident renders (the per-scene scratch rule of the
 * preamble).  One launch with 32-bit work items: RT_ERR_ARG for n above
 *     min(2^30, 64 * floor(0xF0000000 / (64 * C))),  C = the chunk slots per ray at this spp:
 * the samples per item are s = min(64, ceil(spp / B)), B = 24 (BRUTE, GROUPED) or 64 (BVH), and C is
 * ceil(spp / s) rounded up to a power of two; 2^30 rays up to 2 spp, and at 64 spp 125,829,120 rays
 * (BRUTE, GROUPED) or 62,914,560 (BVH).
 */
int rt_render_rays(rt_scene* scene, const rt_ray* rays, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                   uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out);
int rt_render_rays_device(rt_scene* scene, const rt_ray* d_rays, int64_t n, int32_t spp, uint64_t seed,
                          uint64_t sample_base, uint64_t stream_base, double* d_sum, uint32_t* d_samples,
                          uint32_t* d_misses, unsigned long long* d_rays_count, void* stream);

/*
 * Beams: rt_render_rays with anti-aliasing.  All spp samples of a ray of rt_render_rays follow the same
 * ray, so a host's own camera gets converged shading and aliased geometry.  A beam is a ray plus a
 * first-order footprint, how its origin and its direction move across the pixel (or texel, or probe
 * cell) it stands for, and every sample takes its own point (u, v) of the footprint from the two draws
 * GetCameraRay spends on subX and subY, which rt_render_rays discards.  A frustum camera's unnormalised
 * direction and an orthographic camera's origin are linear in the sample point, so both of the library's
 * cameras are beams exactly (rt_camera_beams); for any other camera the beam is its first-order model.
 */
/* 192 B, twelve 16-byte rows.  w components are ignored but must be finite. */
typedef struct rt_beam {
    rt_vec4d origin, direction;          /* the ray at the footprint's corner (u, v) = (0, 0); direction need NOT be unit */
    rt_vec4d origin_du, origin_dv;       /* origin(u, v)    = origin    + u * origin_du    + v * origin_dv    */
    rt_vec4d direction_du, direction_dv; /* direction(u, v) = direction + u * direction_du + v * direction_dv, then normalised */
} rt_beam;
/*
 * Sample k of beam i (normative; F = round to nearest fp32; every fp32 operation is rounded on its own,
 * nothing is contracted into a fused multiply-add):
 *   rng = rt_rng_init(seed, stream_base + i, sample_base + k); u = the first draw * 2^-24, v = the second
 *   draw * 2^-24, both exact in fp32: the draws GetCameraRay spends on subX, subY.
 *   per component c of x, y, z:
 *     o_c = (F(origin_c)    + u * F(origin_du_c))    + v * F(origin_dv_c)
 *     w_c = (F(direction_c) + u * F(direction_du_c)) + v * F(direction_dv_c)
 *   n2 = (w_x * w_x + w_y * w_y) + w_z * w_z
 *   The sample is degenerate if n2 is 0 or not finite, or a component of o is not finite: a primary miss
 *   (misses += 1, nothing added to the sum, no ray counted); the beam's other samples are unaffected.
 *   Otherwise d_c = w_c / sqrt(n2), IEEE square root and IEEE division, and the path is traced from (o, d)
 *   as bounce 0 with the bounce draws following from the third draw on.
 * A beam is invalid if one of its 24 doubles is not finite, or one of the 18 used ones is not after F:
 * all spp samples are then primary misses and no ray is counted (rt_render_rays' rule for a bad ray).
 * So sample k of beam i is, bit for bit, what rt_render_rays returns at spp = 1, sample_base + k and
 * stream_base + i for the ray rt_debug_beam_rays reports for it.
 *
 * Everything else is rt_render_rays' contract with "ray" replaced by "beam": the accumulation into sum,
 * samples, misses and the ray count; the independence of n, list position, chunking and wave (the
 * samples per work item are a function of spp alone); the coherence note; the bound on n of the device
 * entry; always the generic kernels; RT_ERR_STATE on a BVH2 scene; the argument errors, and n == 0
 * returning RT_OK and touching nothing; the counters of rt_scene_get_stats, an armed rt_debug_ray_log,
 * rt_kernel_times and the scene-specialised kernels left as they were; no camera needed.
 * rt_render_beams works in chunks of at most 2^18 beams (RTCORE_QUERY_CHUNK sets a smaller size; fewer
 * when spp is large, as for rt_render_rays), two of them resident: 112 MiB of beams and records on the
 * device and as much pinned staging, in the buffers rt_render_rays uses (there 96 MiB each).
 * Depth of field is not part of a beam: it would take two more draws.
 */
int rt_render_beams(rt_scene* scene, const rt_beam* beams, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                    uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out);
int rt_render_beams_device(rt_scene* scene, const rt_beam* d_beams, int64_t n, int32_t spp, uint64_t seed,
                           uint64_t sample_base, uint64_t stream_base, double* d_sum, uint32_t* d_samples,
                           uint32_t* d_misses, unsigned long long* d_rays_count, void* stream);
/* Host only, no device: the twin.  rays_out[i * spp + k] = the fp32 ray of sample k of beam i, widened
   (origin.w = 1, direction.w = 0); a degenerate sample or invalid beam gives an all-zero origin and direction
   (a miss by rt_render_rays' rule).  uv_out (may be NULL) gets u, v per sample, uv_out[2 * (i * spp + k)]
   and the entry after it.  Returns RT_OK / RT_ERR_ARG (a null pointer with n > 0, n < 0, spp <= 0). */
int rt_debug_beam_rays(const rt_beam* beams, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                       uint64_t stream_base, rt_ray* rays_out, double* uv_out);
/* Host only, no device: the beams of the pixels of a tile for the library's own cameras, out[x*h + y], in fp64
   from Camera.InitRender's state (the function rt_camera_rays uses).
   frustum: origin = position, direction = look + side*offX(x) + up*offY(y)  (GetRay's vector before
            normalisation), direction_du = side * (tanX / w2), direction_dv = up * (tanY / h2), origin_d* = 0;
   ortho:   origin = GetRay(x, y)'s origin, origin_du / origin_dv its step per pixel, direction = look, direction_d* = 0.
   The pinhole footprint: image_plane and depth of field are not represented (documented, not an error).
   RT_ERR_ARG as rt_camera_rays. */
int rt_camera_beams(const rt_camera* camera, int32_t width, int32_t height, int32_t x0, int32_t y0, int32_t w,
                    int32_t h, rt_beam* out);

/*
 * Surfels: the radiance arriving at a surface point, for a lightmap texel, a vertex bake or a light
 * probe.  That is the mean of GetColor over a distribution of directions about a normal; with
 * rt_render_rays the host draws those directions itself and brings one rt_ray per sample.  A surfel is a
 * position and a normal, and every sample draws its own direction on the device from the two draws
 * GetCameraRay spends on subX and subY, which rt_render_rays discards, by the functions the kernels'
 * diffuse bounce runs: one 64-byte record per point instead of one per sample.
 */
/* 64 B, four 16-byte rows.  w components are ignored but must be finite.  The normal need NOT be unit. */
typedef struct rt_surfel {
    rt_vec4d position, normal;
} rt_surfel;
typedef enum rt_gather_mode {
    RT_GATHER_DIFFUSE = 0, /* the reference's diffuse bounce: z = 2 acos(U1) / pi  (Raytracer.cs:215) */
    RT_GATHER_COSINE = 1,  /* Lambert: z = sqrt(1 - U1); the mean is irradiance / pi                  */
    RT_GATHER_SPHERE = 2   /* uniform over the sphere: z = 1 - 2 U1 (a probe; the normal only fixes the frame) */
} rt_gather_mode;
/*
 * Sample k of surfel i (normative; F = round to nearest fp32; fp32 throughout, every operation rounded on
 * its own, and a fused multiply-add only where the kernels' bounce has one):
 *   rng = rt_rng_init(seed, stream_base + i, sample_base + k); U1 = the first draw * 2^-24, U2 = the second
 *   draw * 2^-24, both exact in fp32: the draws rt_render_rays discards.  The bounce draws follow from the
 *   third draw on, as for a ray.
 *   o = F(position), component by component.
 *   n^ = F(normal) / sqrt(n2), n2 = (x * x + y * y) + z * z of F(normal), IEEE square root and IEEE division.
 *   z by mode (above); 2 acos(U1) / pi by the kernels' polynomial, the square roots by the hardware's.
 *   s = sqrt(max(0, 1 - z^2)), 1 - z^2 as one fused multiply-add.
 *   d = n^ z + s (c cos 2 pi U2 + (n^ x c) sin 2 pi U2), c = normalize(n^.y, -n^.x, 0), or (1, 0, 0) when
 *   both components are 0: Vec4D.CreateHorizon in the Rodrigues form of the kernels' diffuse bounce, with
 *   the hardware's sine and cosine (their argument in turns: U2 itself) and reciprocal square root.
 *   Then one Newton step of the normalisation, d (1.5 - 0.5 |d|^2), as a renormalised bounce gets: the ray
 *   meets rt_ray's "already normalised" contract.
 *   The path is traced from (o, d) as bounce 0 with tint 1 and no skip primitive: a caller that leaves a
 *   surface offsets the position itself, as for rt_occluded_rays.
 * A surfel is invalid if one of its 8 doubles is not finite, or one of the 6 used ones is not after F, or
 * n2 is zero or not finite: all spp samples are then primary misses and no ray is counted (rt_render_rays'
 * rule for a bad ray).
 * Two promises:
 *  (a) rt_debug_surfel_rays_device reports the fp32 ray of every sample, and sample k of surfel i is, bit
 *      for bit, what rt_render_rays returns at spp = 1, sample_base + k and stream_base + i for that ray.
 *  (b) that ray is the fp64 evaluation of the formulas above to within the bounds the kernels' bounce
 *      directions are held to (3e-5 per direction component, 5e-7 in length; origin exact).
 *
 * A gather sample that meets nothing is a PRIMARY miss: it is counted in misses and not added to sum.  The
 * reference returns the untinted AmbientRGB for a bounce that misses (Raytracer.cs:90), so the gathered
 * mean is (sum + misses * ambient) / (samples + misses).
 * A gather path has Recursion + 1 segments, one more than the continuation of a rendered diffuse bounce.
 *
 * Everything else is rt_render_rays' contract with "ray" replaced by "surfel": the accumulation into sum,
 * samples, misses and the ray count; the independence of n, list position, chunking and wave (the
 * samples per work item are a function of spp alone); the coherence note; the bound on n of the device
 * entry; always the generic kernels; RT_ERR_STATE on a BVH2 scene; the argument errors, plus RT_ERR_ARG
 * for an unknown mode (checked first), and n == 0 returning RT_OK and touching nothing; the counters of
 * rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels left
 * as they were; no camera needed.  rt_render_surfels works in rt_render_rays' chunks (2^19 surfels,
 * RTCORE_QUERY_CHUNK) in rt_render_rays' buffers: a surfel has an rt_ray's size.
 * Not part of a surfel: a footprint (list several surfels per texel) and a primitive to skip.
 */
int rt_render_surfels(rt_scene* scene, int32_t mode, const rt_surfel* surfels, int64_t n, int32_t spp, uint64_t seed,
                      uint64_t sample_base, uint64_t stream_base, rt_color* sum_rgb, uint32_t* samples,
                      uint32_t* misses, uint64_t* rays_out);
int rt_render_surfels_device(rt_scene* scene, int32_t mode, const rt_surfel* d_surfels, int64_t n, int32_t spp,
                             uint64_t seed, uint64_t sample_base, uint64_t stream_base, double* d_sum,
                             uint32_t* d_samples, uint32_t* d_misses, unsigned long long* d_rays_count, void* stream);
/* The sample rays, by a second compilation of the kernels' function.  No scene: it runs on the calling
   thread's current device, as rt_tonemap_device does, asynchronous on `stream`.  d_rays_out[i * spp + k] =
   the fp32 ray of sample k of surfel i, widened (origin.w = 1, direction.w = 0); an invalid surfel gets all
   zeros (a miss by rt_render_rays' rule).  Returns RT_OK / RT_ERR_ARG (an unknown mode, a null pointer with
   n > 0, n < 0, spp <= 0) / RT_ERR_HIP. */
int rt_debug_surfel_rays_device(int32_t mode, const rt_surfel* d_surfels, int64_t n, int32_t spp, uint64_t seed,
                                uint64_t sample_base, uint64_t stream_base, rt_ray* d_rays_out, void* stream);

/*
 * Light probes: what arrives at a point, kept as a function of direction.  An RT_GATHER_SPHERE gather
 * returns one colour per point, the mean over the sphere; rt_render_probes returns, per point, the sums of
 * its SPHERE gather samples weighted by the nine L2 real spherical-harmonic basis functions of each
 * sample's direction, and the same projection of the directions that met nothing (which never leave the
 * device otherwise).  From them a diffuse receiver's irradiance for any normal is a nine-term dot product.
 *
 * The record.  A probe is an rt_surfel: position is the point, normal only fixes the frame in which the
 * sphere's directions are drawn (RT_GATHER_SPHERE's rule; the mode is fixed).  It is invalid exactly when
 * rt_render_surfels calls it invalid.
 * Sampling (normative).  Sample k of probe i is sample k of surfel i of rt_render_surfels in
 * RT_GATHER_SPHERE: its ray is the one rt_debug_surfel_rays_device reports, and its fp32 colour col and
 * whether it is a primary miss are what rt_render_rays gives for that ray at spp = 1, sample_base + k and
 * stream_base + i.
 * Basis (normative).  (x, y, z) = the reported fp32 direction widened to fp64; fp64 throughout, every
 * operation rounded on its own, no fused multiply-add; the constants are these decimal literals:
 *   K0 = 0.28209479177387814   K1 = 0.48860251190291992   K2 = 1.0925484305920792
 *   K3 = 0.31539156525252005   K4 = 0.54627421529603959
 *   Y0 = K0        Y1 = K1*y      Y2 = K1*z                  Y3 = K1*x       Y4 = (K2*x)*y
 *   Y5 = (K2*y)*z  Y6 = K3*((3*z)*z - 1)                     Y7 = (K2*x)*z   Y8 = K4*(x*x - y*y)
 * Accumulation (normative).  Everything is added to what the arrays hold; per probe in sample order
 * k = 0 .. spp - 1:
 *   a hit:          c[l][j] = c[l][j] + ((double)col_j * Y_l) for j = 0, 1, 2 (r, g, b), the product rounded,
 *                   then the sum; samples += 1
 *   a primary miss: c[l][3] = c[l][3] + Y_l; misses += 1
 *   an invalid probe: misses += spp and nothing else (its rays are all zeros).
 * So c[.][3] is the projection of the probe's view of the sky, and the probe's radiance coefficients are
 *   L[l][ch] = 4 pi / N * (c[l][ch] + c[l][3] * ambient_ch),   N = samples + misses.
 * The ray count follows rt_render_rays.
 * What is promised (normative):
 *   1. The result equals rt_debug_probe_fold over the reported rays and the per-sample rt_render_rays
 *      results, and a replay of the formulas above, bit for bit.
 *   2. A probe's result depends on (seed, stream_base + i, the sample indices, the record, the traversal
 *      mode) only: not on n, on list position, on the host entry's chunking or on the stream.
 *   3. One call of a + b samples equals a call of a samples followed by a call of b samples at
 *      sample_base + a into the same arrays, bit for bit (every work item is one sample at any spp; the
 *      scalar gathers, whose samples per item depend on spp, cannot promise this).
 * Everything else is rt_render_surfels' contract: always the generic kernels; RT_ERR_STATE on a BVH2 scene;
 * the argument errors, and n == 0 returning RT_OK and touching nothing; the counters of rt_scene_get_stats,
 * an armed rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels left as they were; no
 * camera needed; rt_render_probes_device asynchronous on `stream`, ordered like the device-resident renders.
 * Bounds.  One launch holds at most 2^26 work items, one per sample slot: rt_render_probes_device returns
 * RT_ERR_ARG when 64 * ceil(n / 64) * P > 2^26, P = spp rounded up to a power of two; split by n, or by
 * sample_base (promise 3 makes that free).  rt_render_probes takes any n in chunks (2^19 probes,
 * RTCORE_QUERY_CHUNK, fewer where spp asks for it), two of them resident: per probe 360 B up (the record and
 * what the caller's arrays hold, which the sums continue from) and 296 B down; it returns RT_ERR_ARG only
 * when not even 64 probes fit (spp > 2^20).
 */
/* 288 B per probe: nine rows l = 0..8 of four doubles (r, g, b sums and the misses' projection) */
typedef struct rt_probe_sh {
    double c[9][4];
} rt_probe_sh;
int rt_render_probes_device(rt_scene* scene, const rt_surfel* d_probes, int64_t n, int32_t spp, uint64_t seed,
                            uint64_t sample_base, uint64_t stream_base, rt_probe_sh* d_sh, uint32_t* d_samples,
                            uint32_t* d_misses, unsigned long long* d_rays_count, void* stream);
int rt_render_probes(rt_scene* scene, const rt_surfel* probes, int64_t n, int32_t spp, uint64_t seed,
                     uint64_t sample_base, uint64_t stream_base, rt_probe_sh* sh, uint32_t* samples, uint32_t* misses,
                     uint64_t* rays_out);
/* Host only, no device: y9_out[9 i + l] = Y_l of the direction dirs_xyz[3 i ..], the kernel's function
   compiled for the CPU.  RT_ERR_ARG for n < 0 or a null pointer with n > 0. */
int rt_debug_sh_basis(const double* dirs_xyz, int64_t n, double* y9_out);
/* Host only, no device: the accumulation above for n probes of spp samples each, sample k of probe i at
   i * spp + k: its ray (a direction of all zeros: a sample of an invalid probe), its fp32 colour rgb[3 (i spp
   + k) ..] and miss[i spp + k] != 0 for a primary miss; added into sh, samples and misses (n each).
   RT_ERR_ARG for n < 0, spp <= 0 or a null pointer with n > 0. */
int rt_debug_probe_fold(const rt_ray* rays, const float* rgb, const uint8_t* miss, int64_t n, int32_t spp,
                        rt_probe_sh* sh, uint32_t* samples, uint32_t* misses);

/*
 * Adaptive light probes: more samples of only the listed probes of a resident array, with the second
 * moments of each probe's band-0/1 luminance coefficients, and the pass that turns those into the next list --
 * what rt_render_pixels and rt_adaptive_select_device are to a frame.  A probe in a closed, evenly lit corner
 * then stops after a fraction of the samples a probe beside a light needs.  A probe's work item is exactly
 * one sample, so unlike rt_render_list's batch moments these are exact per-sample sums, independent of spp,
 * and the misses' share is kept apart from the ambient colour as c[.][3] keeps it apart in the sums.
 *
 * The moments (normative).  rt_probe_moments rows l = 0 .. 3 are bands 0 and 1, in the order of Y0 .. Y3.
 * Everything is added to what the array holds, per probe in sample order, fp64, every operation rounded on
 * its own, no fused multiply-add; the direction and Y are the fold's:
 *   a hit:          y = (0.299 * (double)col_r + 0.587 * (double)col_g) + 0.114 * (double)col_b, left to right
 *                   (rt_render_pixels' Y_j);  x = y * Y_l;  m[l][0] = m[l][0] + x * x, the product rounded,
 *                   then the sum
 *   a primary miss: m[l][1] = m[l][1] + Y_l * Y_l
 *   a sample of an invalid probe adds nothing.
 * Column 1 stays free of the ambient colour: a hit and a miss are disjoint, so the sum of squares of
 * x_l = Y_l * (hit ? y : A) is m[l][0] + A * A * m[l][1] for any ambient luminance A.
 *
 * rt_render_probe_list_device: rt_render_probes_device for a list of entry numbers into n_records probes
 * resident at d_probes.  d_index holds n entries e = d_index[j]; NULL is the identity list, and n must then
 * equal n_records.  Everything is added at entry e: d_sh, d_samples, d_misses and d_moments (which may be
 * NULL) have n_records elements.  Sample k of entry e draws from (seed, stream_base + e, sample_base + k): it
 * is rt_render_probes' sample k of probe e.
 * What is promised (normative):
 *   1. With the identity list and no moments, the result is rt_render_probes_device's bit for bit from equal
 *      accumulator contents.
 *   2. d_sh, d_samples, d_misses and the ray count are the same with and without d_moments.
 *   3. d_moments equals rt_debug_probe_moments over the reported rays and the per-sample rt_render_rays
 *      results (rt_debug_probe_fold's inputs), bit for bit.
 *   4. An entry's accumulators depend on (seed, stream_base + e, the sample indices, the record, the traversal
 *      mode) only: not on n, on n_records, on the entry's place in the list or on the stream.
 *   5. One call of a + b samples equals a call of a samples followed by a call of b samples at
 *      sample_base + a, bit for bit, moments included.
 *   6. An entry >= n_records is skipped: not traced, nothing written.  An entry named twice is undefined (its
 *      accumulators are updated by two threads).
 * Bounds and errors.  rt_render_probes_device's with n as the list length: RT_ERR_ARG for a null scene, n < 0,
 * spp <= 0; then, for n > 0, a null d_probes, d_sh, d_samples or d_misses, n_records <= 0, n_records >= 2^32,
 * a null index with n != n_records, and 64 * ceil(n / 64) * P > 2^26, P = spp rounded up to a power of two.
 * RT_ERR_STATE on a BVH2 scene.  n == 0 returns RT_OK and touches nothing.  Always the generic kernels; the
 * counters of rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels
 * are left as they were; no camera needed; asynchronous on `stream`, ordered like the device-resident renders.
 * Not part of it: an entry over host buffers.  The adaptive loop is device-resident by nature (its list never
 * leaves the device), and rt_render_probes stays the host entry.
 *
 * The rule (normative).  Everything is fp64, every operation is rounded on its own, division and square root
 * are IEEE.  With a probe's c = rt_probe_sh, m = rt_probe_moments, samples, misses, and the parameters P:
 *   N  = samples + misses (64 bits), n = (double)N
 *   A  = (0.299 * ambient.r + 0.587 * ambient.g) + 0.114 * ambient.b          AA = A * A
 *   for l = 0 .. 3:
 *     S_l = ((0.299 * c[l][0] + 0.587 * c[l][1]) + 0.114 * c[l][2]) + A * c[l][3]
 *     T_l = m[l][0] + AA * m[l][1]
 *     u_l = T_l - (S_l * S_l) / n      d_l = u_l / (n - 1.0)
 *     v_l = u_l > (n * 2^-49) * T_l ? d_l : 0   (so 0 for a NaN)
 *   The guard: T_l and S_l^2 / n are each n rounded additions and differ by up to (3 n + 13) 2^-53 T_l of rounding
 *   alone; a difference not above n 2^-49 T_l is that rounding and not variance.  A probe whose coefficient l is the
 *   same for every sample has v_l = 0 exactly; a relative variance below n 2^-49 cannot be told from it.
 *   a0 = 3.141592653589793 * K0     a1 = 2.0943951023931953 * K1     p4 = 4.0 * 3.141592653589793
 *   level = ((p4 * a0) * S_0) / n
 *   se    = p4 * sqrt(((a0 * a0) * v_0 + (a1 * a1) * ((v_1 + v_2) + v_3)) / n)
 * level is the luminance of the irradiance the probe gives averaged over all normals; se estimates the
 * standard error of the band-0/1 irradiance a diffuse receiver reads, with the covariances between the
 * coefficients left out: an estimate, not a bound.  active(probe) is, in this order:
 *   1. N < min_samples   -> 1
 *   2. N >= max_samples  -> 0
 *   3. N < 2             -> 1
 *   4. a d_l is NaN      -> 0
 *   5. otherwise  se > rel_tol * (level > irr_floor ? level : irr_floor)
 * So a NaN in c[0..3] or in m makes the probe inactive: it cannot converge, so it is not sampled for ever.  An
 * invalid probe (all misses in no direction: c = m = 0) has se = 0 and stops at min_samples.
 * rt_probe_select_device: the active entries' numbers into d_list in ascending order, from accumulators of
 * n_records probes, on the calling thread's current device, asynchronous on `stream`.  *d_count receives the
 * number of active entries, also when it exceeds cap; then only the first cap are stored.  Deterministic as
 * rt_adaptive_select_device (a ballot per 64 entries, an exclusive scan, the write by ballot prefix), whose
 * per-device temporary counts it shares; calls on one device are serialised by the caller.  RT_ERR_ARG for a
 * null pointer (d_list may be NULL with cap = 0), rel_tol NaN or negative, irr_floor NaN or not above 0,
 * n_records <= 0 or >= 2^32.
 * rt_debug_probe_select: the host twin (host only): the same arguments on host arrays, the same rule
 * function; returns the count (at most cap entries stored), or a negative rt_status.
 * rt_debug_probe_error: host only; se_out[i] and level_out[i] of probe i as step 5 reads them, a quiet NaN
 * each where N < 2.  RT_ERR_ARG for a null params, n < 0 or a null pointer with n > 0.
 */
typedef struct rt_probe_moments {   /* 64 B per probe */
    double m[4][2];                 /* [l][0]: hits' sum of (y Y_l)^2; [l][1]: primary misses' sum of Y_l^2 */
} rt_probe_moments;
typedef struct rt_probe_select_params {   /* 48 B */
    double   rel_tol;      /* converged when se <= rel_tol * max(level, irr_floor)                  */
    double   irr_floor;    /* > 0; keeps dark probes from never converging                          */
    rt_color ambient;      /* the ambient colour rt_probe_radiance_device is given for these probes */
    uint32_t min_samples;  /* a probe with N < min_samples is always active                         */
    uint32_t max_samples;  /* a probe with N >= max_samples is never active                         */
} rt_probe_select_params;
int rt_render_probe_list_device(rt_scene* scene, const rt_surfel* d_probes, int64_t n_records, const uint32_t* d_index,
                                int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base,
                                rt_probe_sh* d_sh, uint32_t* d_samples, uint32_t* d_misses,
                                rt_probe_moments* d_moments /* may be NULL */, unsigned long long* d_rays_count,
                                void* stream);
/* Host only, no device: the moments above over rt_debug_probe_fold's inputs (same layout and conventions),
   added into moments (n).  RT_ERR_ARG for n < 0, spp <= 0 or a null pointer with n > 0. */
int rt_debug_probe_moments(const rt_ray* rays, const float* rgb, const uint8_t* miss, int64_t n, int32_t spp,
                           rt_probe_moments* moments);
int rt_probe_select_device(const rt_probe_select_params* params, const rt_probe_sh* d_sh, const uint32_t* d_samples,
                           const uint32_t* d_misses, const rt_probe_moments* d_moments, int64_t n_records,
                           uint32_t* d_list, uint32_t cap, uint32_t* d_count, void* stream);
int64_t rt_debug_probe_select(const rt_probe_select_params* params, const rt_probe_sh* sh, const uint32_t* samples,
                              const uint32_t* misses, const rt_probe_moments* moments, int64_t n_records,
                              uint32_t* list, uint32_t cap);
int rt_debug_probe_error(const rt_probe_select_params* params, const rt_probe_sh* sh, const uint32_t* samples,
                         const uint32_t* misses, const rt_probe_moments* moments, int64_t n, double* se_out,
                         double* level_out);

/*
 * Probe grids: the irradiance a regular grid of such probes gives at shading points, on the device.  Per
 * point: the trilinear blend of the radiance coefficients of its cell's eight probes, without the probes the
 * point cannot see (a probe behind a wall does not light the point in front of it), then the nine-term dot
 * product with the cosine lobe for the point's normal.  A grid goes from rt_render_probes to shading with
 * nothing leaving the device.
 *
 * The grid.  Probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix, x fastest, and the position
 * origin + (ix, iy, iz) * step.  Its radiance is L: n_probes x 9 x 3 doubles, L[p][l][ch].
 *
 * Everything below is normative and fp64: every operation is rounded on its own, nothing is contracted,
 * division and square root are IEEE, no library function is called.
 *
 * Radiance (rt_probe_radiance_device, rt_debug_probe_radiance).  N = samples + misses in 64 bits,
 *   k = (4.0 * 3.141592653589793) / (double)N,   L[l][ch] = k * (c[l][ch] + c[l][3] * ambient_ch),
 * the product rounded, then the sum, then the product by k.  N == 0: all 27 coefficients are a quiet NaN;
 * such a probe is ABSENT.
 * Point.  An rt_surfel.  It is invalid if one of its 8 doubles is not finite, or n2 = (nx*nx + ny*ny) + nz*nz
 * is 0 or not finite: irradiance (0, 0, 0), weight 0, all eight segments zero.  Else n^ = normal / sqrt(n2),
 * component by component.
 * Cell, per axis a.  dims_a == 1: i_a = 0, f_a = 0.  Else g = (p_a - origin_a) / step_a, held to
 * [0, dims_a - 1] (g < 0 ? 0 : g > dims_a - 1 ? dims_a - 1 : g: a point outside the grid takes the boundary's
 * value), i_a = (int)g held to dims_a - 2, f_a = g - (double)i_a.
 * Corners c = dx + 2 dy + 4 dz, c = 0 .. 7.  w_a = d_a ? f_a : 1 - f_a, t_c = (w_x * w_y) * w_z.  A corner
 * with t_c == 0 is NOT VISITED (so no index past dims is formed, and a point at a probe's own position reads
 * that probe alone).  A visited corner's probe is (i_x + dx, i_y + dy, i_z + dz), at
 * q_a = origin_a + (double)(i_a + d_a) * step_a.
 * Segment of point i, corner c, stored at 8 i + c; it depends on the grid and the point only.  A corner that
 * is not visited, or a grid without RT_PROBE_GRID_VISIBILITY: an all-zero rt_ray and t_max = 0, an empty
 * segment, for which rt_occluded_rays answers 0.  Else o_a = p_a + bias * n^_a, v = q - o,
 * d2 = (vx*vx + vy*vy) + vz*vz, dist = sqrt(d2); dist not > 0 or not finite: the empty segment again; else
 * origin = (o, 1), direction = (v / dist, 0), t_max = dist.
 * Visibility.  Corner c is HIDDEN exactly when rt_occluded_rays_device(RT_QUERY_FAST) answers 1 for that
 * segment on this scene in its traversal mode; rt_occluded_rays' rules apply word for word (fp32 rounding of
 * ray and t_max, culling of one-sided primitives, generic kernels only, RTCORE_OCCLUDED_EARLY, RT_ERR_STATE
 * on a BVH2 scene).  Without the flag no query runs and the scene is used only for its device and scratch.
 * Blend, corners ascending; a corner contributes if it is visited, not hidden and present (all 27 of its
 * coefficients finite):  W = W + t_c;  B[l][ch] = B[l][ch] + t_c * L_c[l][ch], the product rounded, then the
 * sum; both start at 0.
 * W > 0:  Y = the basis of "light probes" at n^;  a_l = A_l * Y_l with A_0 = 3.141592653589793,
 * A_1..3 = 2.0943951023931953, A_4..8 = 0.7853981633974483;
 *   E_ch = (a_0 * B[0][ch] + a_1 * B[1][ch] + ... + a_8 * B[8][ch]) / W, left to right.
 * The irradiance is E and the weight W: about 1 when every corner contributes, else the share of the
 * trilinear weight that could see the point.  W == 0: irradiance 0 and weight 0; the caller falls back, for
 * example to a gather at those points.
 * What is promised:
 *   1. The device result equals rt_debug_shade_probes fed with rt_debug_probe_segments_device's segments and
 *      rt_occluded_rays_device's answers for them, bit for bit.
 *   2. The device segments equal rt_debug_probe_segments, bit for bit.
 *   3. A point's result depends on the grid, L, the record and the traversal mode only: not on n, on list
 *      position, on chunking or on the stream.
 * Calls.  `grid` is always a host pointer, copied by value into the launches.  The outputs are written, not
 * added to; d_weight / weight may be NULL.  RT_ERR_ARG, before anything is launched, for a null scene or
 * grid; a grid that breaks a rule of the struct; n < 0; then, for n > 0, a null L, points or irradiance
 * pointer.  n == 0 returns RT_OK and touches nothing.  RT_ERR_STATE on a BVH2 scene only with the visibility
 * flag.  No camera is needed; the counters of rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times
 * and the scene-specialised kernels are left as they were.  rt_shade_probes_device is asynchronous on
 * `stream`, ordered like the device-resident renders, and works in chunks of 2^16 points (RTCORE_QUERY_CHUNK
 * / 8: one any-hit launch of at most 2^19 segments, 73 B of per-scene scratch each); rt_shade_probes uploads
 * L once and takes the points in the same chunks, 64 B up and 32 B down per point.
 * Not part of it: DDGI's backface "wrap" weight and its Chebyshev depth moments (these are "probe depth
 * maps", below: rt_shade_probes_depth_device); a shortened segment end (probes belong in the air);
 * RT_QUERY_EXACT; a grid that is not axis-aligned; adding into the outputs.
 */
#define RT_PROBE_GRID_VISIBILITY 1u
typedef struct rt_probe_grid {   /* 80 B, five 16-byte rows */
    double   origin[3];  /* position of probe (0, 0, 0); finite                                */
    double   step[3];    /* spacing per axis; finite and > 0 (also where dims is 1)             */
    int32_t  dims[3];    /* nx, ny, nz >= 1; nx * ny * nz < 2^31                                */
    uint32_t flags;      /* RT_PROBE_GRID_VISIBILITY: leave out the probes the point cannot see */
    double   bias;       /* finite, >= 0: the segments start at position + bias * unit normal   */
    uint32_t reserved[2];/* 0 */
} rt_probe_grid;
/* L from rt_render_probes' accumulators, on the calling thread's current device (as rt_tonemap_device),
   asynchronous on `stream`.  RT_ERR_ARG for n < 0, n >= 2^31 or a null pointer with n > 0. */
int rt_probe_radiance_device(const rt_probe_sh* d_sh, const uint32_t* d_samples, const uint32_t* d_misses, int64_t n,
                             rt_color ambient, double* d_L, void* stream);
/* Its host twin: host only, no device. */
int rt_debug_probe_radiance(const rt_probe_sh* sh, const uint32_t* samples, const uint32_t* misses, int64_t n,
                            rt_color ambient, double* L);
int rt_shade_probes_device(rt_scene* scene, const rt_probe_grid* grid, const double* d_L, const rt_surfel* d_points,
                           int64_t n, rt_color* d_irradiance, double* d_weight, void* stream);
int rt_shade_probes(rt_scene* scene, const rt_probe_grid* grid, const double* L, const rt_surfel* points, int64_t n,
                    rt_color* irradiance, double* weight);
/* The eight segments of every point (no scene: the current device, as rt_debug_surfel_rays_device), and the
   host twin.  RT_ERR_ARG as above, and for a null output pointer with n > 0. */
int rt_debug_probe_segments_device(const rt_probe_grid* grid, const rt_surfel* d_points, int64_t n, rt_ray* d_rays_out,
                                   double* d_t_max_out, void* stream);
int rt_debug_probe_segments(const rt_probe_grid* grid, const rt_surfel* points, int64_t n, rt_ray* rays_out,
                            double* t_max_out);
/* Host twin of the blend, no device: occluded = rt_occluded_rays' answers for those segments (n * 8 bytes),
   NULL = all 0. */
int rt_debug_shade_probes(const rt_probe_grid* grid, const double* L, const rt_surfel* points, int64_t n,
                          const uint8_t* occluded, rt_color* irradiance, double* weight);

/*
 * Probe depth maps: the visibility of a probe grid without a ray at shading time.  The grid's
 * RT_PROBE_GRID_VISIBILITY traces eight any-hit segments per shading point; here the bake stores, with every
 * probe, an octahedral map of the first two moments of the distance it sees, and the shading pass weighs each
 * corner of a point's cell by a one-sided Chebyshev bound on "the probe sees at least this far in the point's
 * direction" (DDGI's visibility test), optionally times DDGI's backface "wrap" weight.  It traces no ray, keeps
 * no scratch and needs no scene.  The bake also counts the samples that met a back face (rt_hit.inside): a
 * probe with a large share of them sits inside geometry.
 *
 * Everything below is normative and fp64 as "probe grids" is: every operation rounded on its own, nothing
 * contracted, IEEE division and square root, no library function.  sgn(a) = a >= 0 ? 1 : -1 (so sgn(-0.0) = 1).
 *
 * The map.  R = 8; texel t = ty * 8 + tx, 64 per probe.
 * Direction T_t of a texel:  u = (double)(2 tx + 1) / 8 - 1, v likewise (both exact);  z = (1 - |u|) - |v|;
 *   z < 0:  x = (1 - |v|) * sgn(u),  y = (1 - |u|) * sgn(v);  else x = u, y = v;
 *   T = (x, y, z) / sqrt((x*x + y*y) + z*z), component by component.
 * Texel of a vector (x, y, z), finite and not zero, of any length:  s1 = (|x| + |y|) + |z|,  u = x / s1,
 *   v = y / s1;  z < 0:  u' = (1 - |v|) * sgn(x),  v' = (1 - |u|) * sgn(y);  else u' = u, v' = v;
 *   tx = (int)((u' + 1) * 4) held to [0, 7], ty likewise from v'.  The texel of T_t is t.
 * Accumulators, rt_probe_depth: s[0][t] = sum of w, s[1][t] = sum of w d, s[2][t] = sum of w d^2.
 * Counts, four uint32 per probe: hits, hits with rt_hit.inside != 0 (these are hits too), misses, skipped.
 *
 * The bake (rt_render_probe_depth_device).  Sample k of probe i is sample k of surfel i of "radiance queries"
 * in RT_GATHER_SPHERE mode: its ray is the one rt_debug_surfel_rays_device reports for (seed, sample_base,
 * stream_base), so a depth bake and an rt_render_probes bake with the same three look in the same directions;
 * its hit is what rt_query_rays_device(RT_QUERY_FAST) answers for that ray on this scene in its traversal
 * mode.  Added to what the arrays hold, per probe in sample order k = 0 .. spp - 1:
 *   a direction of all zeros (an invalid probe):  skipped += 1, nothing else;
 *   else  d = hit (prim_id >= 0) and distance < d_max ? distance : d_max;  hits (and inside hits) or misses += 1;
 *   for every texel t, with (x, y, z) the ray's direction:  c = (x * T_x + y * T_y) + z * T_z;  c not > 0 adds
 *   nothing;  else w = c squared `sharpness` times (w = w * w),
 *     s[0][t] += w;   s[1][t] += w * d;   s[2][t] += (w * d) * d,   each product rounded, then each sum.
 * What is promised:
 *   1. The device result equals rt_debug_probe_depth_fold over the reported rays and the query's answers, bit
 *      for bit.
 *   2. A probe's result depends on (seed, stream_base + i, the sample indices, the record, the params, the
 *      traversal mode) only: not on n, on list position, on chunking or on the stream.
 *   3. A call of a + b samples equals a call of a samples followed by one of b samples at sample_base + a into
 *      the same arrays, bit for bit.
 * Calls.  `params` is a host pointer.  RT_ERR_ARG, before anything is launched, for what rt_render_probes_device
 * refuses (a null scene, n < 0, spp <= 0, then for n > 0 a null pointer), for params that break a rule of the
 * struct and for spp > 2^19 (split by sample_base).  n == 0 returns RT_OK and touches nothing.  RT_ERR_STATE on
 * a BVH2 scene.  Always the generic kernels; no camera is needed; the counters of rt_scene_get_stats, an armed
 * rt_debug_ray_log, rt_kernel_times and the scene-specialised kernels are left as they were.  Asynchronous on
 * `stream`, ordered like the device-resident renders; chunks of max(1, 2^19 / spp) whole probes
 * (RTCORE_QUERY_CHUNK samples), 64 + 48 B of per-scene scratch per sample.  No host-buffer entry.
 *
 * The close (rt_probe_depth_close_device).  D: n x 64 x 2 doubles, D[p][t] = (s[1][t] / s[0][t],
 * s[2][t] / s[0][t]) = (mu, m2); where s[0][t] is not > 0 both are a quiet NaN.  A texel one of whose two
 * values is not finite is ABSENT.
 *
 * The shading (rt_shade_probes_depth_device).  The grid is "probe grids"' with flags == 0.  Point, cell,
 * corners and t_c are exactly that section's.  For each visited corner, with the probe's position q and
 * o_a = p_a + bias * n^_a as its segments form them:  v = o - q,  r = sqrt((vx*vx + vy*vy) + vz*vz).
 *   r not > 0 or not finite:  c = 1, wrap = 1.
 *   else  (mu, m2) = D[probe][texel of v],  r_c = r < d_max ? r : d_max;
 *     the texel absent, or r_c not > mu:  c = 1;
 *     else  var = m2 - mu * mu,  var = var > var_floor ? var : var_floor,  delta = r_c - mu,
 *           c = var / (var + delta * delta),  then c = (c * c) * c;
 *     with RT_PROBE_DEPTH_WRAP:  h = (1 - ((vx * n^x + vy * n^y) + vz * n^z) / r) * 0.5,  wrap = h * h + 0.2
 *     (1.2 for a normal that faces the probe, 0.2 for one that faces away);  without it wrap = 1.
 *   t' = (t_c * c) * wrap.
 * Blend: that section's, corners ascending, with t' in place of t_c over the corners that are visited, present
 * and have t' > 0:  W = W + t',  B = B + t' * L_c;  the irradiance formula is the same; W == 0 gives
 * irradiance 0 and weight 0.
 * What is promised:
 *   1. The device result equals rt_debug_shade_probes_depth, bit for bit.
 *   2. A point's result depends on the grid, the params, L, D and the record only.
 *   3. With every texel of D absent and no wrap flag the result equals rt_shade_probes_device on the same grid
 *      (flags 0), bit for bit (t_c * 1 is exact).
 * Calls.  grid and params are host pointers.  Both entries run on the calling thread's current device, as
 * rt_probe_radiance_device does.  RT_ERR_ARG, before anything is launched, for a null grid or params, a grid
 * or params that break a rule of their struct, grid flags other than 0 (RT_PROBE_GRID_VISIBILITY included),
 * n < 0, then for n > 0 a null L, D, points or irradiance pointer; n == 0 returns RT_OK and touches nothing.
 * The close: RT_ERR_ARG for n < 0, n >= 2^25 or a null pointer with n > 0.  Outputs are written, not added to;
 * d_weight may be NULL.
 * Not part of it: a host-buffer bake; bilinear lookup across the octahedral seams; fusing the fold into
 * rt_render_probes' launch.  (Relocation, which the backface share drives, is "probe relocation" below.)
 */
#define RT_PROBE_DEPTH_WRAP 1u
typedef struct rt_probe_depth_params {   /* 32 B */
    double   d_max;       /* finite, > 0: distances are held to it; a miss counts as d_max       */
    double   var_floor;   /* finite, > 0: the least variance the Chebyshev test works with       */
    int32_t  sharpness;   /* 0 .. 8: a sample's weight in a texel is its cosine squared this often */
    uint32_t flags;       /* RT_PROBE_DEPTH_WRAP: the shading multiplies by the wrap weight      */
    uint32_t reserved[2]; /* 0 */
} rt_probe_depth_params;
typedef struct rt_probe_depth {   /* 1536 B per probe: three rows of 64 texels, texel index fastest */
    double s[3][64];
} rt_probe_depth;
int rt_render_probe_depth_device(rt_scene* scene, const rt_surfel* d_probes, int64_t n, int32_t spp, uint64_t seed,
                                 uint64_t sample_base, uint64_t stream_base, const rt_probe_depth_params* params,
                                 rt_probe_depth* d_depth, uint32_t* d_counts, void* stream);
/* Its fold on the host, no device: rays and hits are n * spp of each, probe i's at [i * spp, (i + 1) * spp). */
int rt_debug_probe_depth_fold(const rt_probe_depth_params* params, const rt_ray* rays, const rt_hit* hits, int64_t n,
                              int32_t spp, rt_probe_depth* depth, uint32_t* counts);
int rt_probe_depth_close_device(const rt_probe_depth* d_depth, int64_t n, double* d_D, void* stream);
int rt_debug_probe_depth_close(const rt_probe_depth* depth, int64_t n, double* D);
int rt_shade_probes_depth_device(const rt_probe_grid* grid, const rt_probe_depth_params* params, const double* d_L,
                                 const double* d_D, const rt_surfel* d_points, int64_t n, rt_color* d_irradiance,
                                 double* d_weight, void* stream);
int rt_debug_shade_probes_depth(const rt_probe_grid* grid, const rt_probe_depth_params* params, const double* L,
                                const double* D, const rt_surfel* points, int64_t n, rt_color* irradiance, double* weight);
/* The two texel rules on the host: the 64 directions T_t as 64 x 3 doubles; the texels of n vectors (3 doubles
   each; -1 for one that is zero or not finite). */
int rt_debug_oct_texel_dirs(double* dirs_out);
int rt_debug_oct_texel(const double* vectors_xyz, int64_t n, int32_t* texels_out);

/*
 * Probe relocation: per-probe offsets that move a grid's probes off nearby geometry, a device pass that
 * derives them from the hit distances of a probe's own sample directions and classifies the probe (DDGI's
 * relocation and classification), and shading entries that honour the offsets and states.  A grid alone can
 * place a probe only at origin + i * step; a probe next to a wall sees it under a wide range of distances
 * inside one texel of its depth map, and the Chebyshev test then hides little ("probe depth maps").
 *
 * Everything below is normative and fp64 as "probe grids" is: every operation rounded on its own, nothing
 * contracted, IEEE division and square root, no library function.  A comparison with a NaN is false.
 *
 * Placement.  Offsets: n_probes x 3 doubles in world units, indexed like L; a NULL pointer means all zero.
 * State: n_probes uint32, bits RT_PROBE_INSIDE and RT_PROBE_IDLE; a NULL pointer means all 0.  The position of
 * probe (i_x, i_y, i_z) is  q_a = (origin_a + (double)i_a * step_a) + offset_a:  the grid term is "probe
 * grids"', the offset is added last (also a zero offset, for a NULL pointer +0.0).  An offset is valid when its
 * three components are finite; a probe with a non-finite offset is ABSENT everywhere below.
 * rt_probe_positions_device writes one rt_surfel per grid probe, in index order: position (q, 1), normal
 * (0, 0, 1, 0); for a non-finite offset the position is four quiet NaNs, an invalid surfel for every entry.
 * This is the array rt_render_probes_device, rt_render_probe_list_device and rt_render_probe_depth_device take,
 * so the three bakes work at relocated positions unchanged.
 *
 * One relocation step (rt_relocate_probes_device).  Sample k of probe i is sample k of surfel i of
 * rt_probe_positions_device's array in RT_GATHER_SPHERE mode, keyed (seed, stream_base + i, sample_base + k):
 * the ray rt_debug_surfel_rays_device reports; its hit is rt_query_rays_device(RT_QUERY_FAST)'s answer on this
 * scene in its traversal mode: the directions and the query of the depth bake.  d is rt_hit.distance.
 * The fold, per probe, over k = 0 .. spp - 1, from (d_near, k_near) = (+inf, -1), (d_back, k_back) = (+inf, -1),
 * (d_far, k_far) = (-inf, -1) and all counts 0:
 *   a direction of all zeros:      skipped += 1;
 *   a miss (prim_id < 0):          misses += 1;
 *   a hit with inside != 0:        back += 1;   d < d_back:  (d_back, k_back) = (d, k);
 *   any other hit:                 front += 1;  d < d_near:  (d_near, k_near) = (d, k);
 *                                               d > d_far:   (d_far, k_far) = (d, k).
 * Ties therefore keep the lowest k, and a NaN distance is counted and never chosen.
 * The rule.  o is the offset read, D_k the reported direction of sample k (fp32 values in doubles; (0, 0, 0)
 * for k = -1), hits = back + front, s the grid's step.
 *   (a) hits > 0 and (double)back > back_share * (double)hits:
 *         m = d_back + min_front * 0.5,   c_a = o_a + D_kback,a * m;   state bit RT_PROBE_INSIDE.
 *   (b) else front > 0 and d_near < min_front:
 *         p = (Dn_x * Df_x + Dn_y * Df_y) + Dn_z * Df_z  with Dn = D_knear, Df = D_kfar;
 *         p > 0:  c = o  (moving toward the far surface would also approach the near one);
 *         else    h = d_far * 0.5,  t = h < min_front ? h : min_front,  c_a = o_a + Df_a * t  (the probe never
 *                 passes the far surface).
 *   (c) else (nothing near: move home):
 *         len = sqrt((o_x * o_x + o_y * o_y) + o_z * o_z);   len not > 0:  c = o;
 *         else  room = (front > 0 ? d_near : +inf) - min_front,  m = room < len ? room : len;
 *               m == len:  c = (+0.0, +0.0, +0.0);   else  c_a = o_a - (o_a / len) * m.
 *   Accept:  e_a = c_a / s_a.  c becomes the offset when its three components are finite and
 *         (e_x * e_x + e_y * e_y) + e_z * e_z < max_offset * max_offset;  otherwise the offset stays o.
 *   State bit RT_PROBE_IDLE:  front == 0, or d_near > sqrt((s_x * s_x + s_y * s_y) + s_z * s_z): no front face
 *         within the cell's diagonal, so no surface is there to shade from this probe.  It is information for the
 *         baker, who feeds the other probes to rt_render_probe_list_device; shading does not act on it.
 *   A probe whose samples were all skipped (an invalid position):  the offset stays, state = RT_PROBE_INSIDE |
 *         RT_PROBE_IDLE, moved = 0.
 * rt_probe_relocation, per probe: the state, the counts, the three winners, and moved = 1 when the bits of the
 * offset the rule gives differ from those of o.  With RT_PROBE_RELOCATE_CLASSIFY_ONLY the record is the same
 * (moved reports what a step would do) and the offsets are read, never written.
 * What is promised:
 *   1. The device result (offsets and records) equals rt_debug_probe_relocate over the reported rays and the
 *      query's answers, bit for bit.  (The device folds a probe's samples across the lanes of a wave and reduces
 *      (d, k) pairs in the lexicographic order "smaller d, then smaller k" (far: larger d, then smaller k), which
 *      is what the sequential fold with strict comparisons selects.)
 *   2. A probe's result depends on its grid position, its offset, the params, (seed, stream_base + i, the sample
 *      indices) and the traversal mode only: not on chunking or on the stream.
 *   3. With RT_PROBE_RELOCATE_CLASSIFY_ONLY, d_offsets is bit-identical afterwards.
 * Calls.  grid and params are host pointers; the grid's flags and bias play no part.  RT_ERR_ARG, before
 * anything is launched, for a null scene, grid or params, a grid or params that break a rule of their struct,
 * spp <= 0, spp > 2^19 (take several steps), a null d_offsets or d_info.  RT_ERR_STATE on a BVH2 scene.  Always
 * the generic kernels; no camera is needed; the counters of rt_scene_get_stats, an armed rt_debug_ray_log,
 * rt_kernel_times and the scene-specialised kernels are left as they were.  Asynchronous on `stream`, ordered
 * like the device-resident renders; chunks of max(1, 2^19 / spp) whole probes (RTCORE_QUERY_CHUNK samples),
 * 64 + 48 B of per-scene scratch per sample (the depth bake's) and 64 B per probe of a chunk.
 *
 * Shading that honours the placement.  The _placed entries take offsets and state after the grid and are
 * otherwise their unplaced entries, word for word: cell, corners and t_c stay the grid's (the trilinear weights
 * belong to the lattice, as in DDGI); only q changes, so the segments' ends, and the depth shading's v, r and
 * texel, change with it.  A probe with state & RT_PROBE_INSIDE, or with a non-finite offset, is ABSENT: it is
 * not blended, and its segment is the empty one.
 * What is promised:
 *   1. Device equals twin, bit for bit, as for the unplaced entries.
 *   2. With NULL offsets and NULL state, and with all-zero arrays, every placed entry's result equals its
 *      unplaced entry's, bit for bit.  (x + 0.0 is exact but -0.0 + 0.0 is +0.0: only the bits of q can differ
 *      there, and only in the sign of a zero.  The grid term is in fact never -0.0: (double)i_a * step_a is +0.0
 *      or above 0, and a sum is -0.0 only when both terms are; so the results agree in every bit.)
 * Calls.  As the unplaced entries; offsets and state are device pointers in the _device entries and host
 * pointers in the others, each may be NULL.  rt_shade_probes_placed uploads them once, with L.
 * Not part of it: moving the cell or the trilinear weights with the probes; acting on RT_PROBE_IDLE in the
 * shading; a relocation over host buffers.
 */
#define RT_PROBE_INSIDE 1u                 /* state: the probe sits inside geometry; absent in the shading */
#define RT_PROBE_IDLE 2u                   /* state: no front face within the cell's diagonal              */
#define RT_PROBE_RELOCATE_CLASSIFY_ONLY 1u /* params.flags: offsets are read, never written                */
typedef struct rt_probe_relocate_params {   /* 32 B */
    double   back_share;  /* finite, in [0, 1): the share of back-face hits above which a probe is inside (DDGI: 0.25) */
    double   min_front;   /* finite, > 0, world units: the clearance a probe keeps from a front face                  */
    double   max_offset;  /* finite, in (0, 0.5): the offset's bound, in steps, an ellipsoid (DDGI: 0.45)             */
    uint32_t flags;       /* RT_PROBE_RELOCATE_CLASSIFY_ONLY or 0 */
    uint32_t reserved;    /* 0 */
} rt_probe_relocate_params;
typedef struct rt_probe_relocation {   /* 64 B */
    uint32_t state, moved, front, back, misses, skipped;
    int32_t  k_near, k_back, k_far, reserved;   /* -1: none; reserved 0 */
    double   d_near, d_back, d_far;             /* +inf, +inf, -inf: none */
} rt_probe_relocation;
/* On the calling thread's current device (as rt_probe_radiance_device), asynchronous on `stream`; d_offsets may
   be NULL.  RT_ERR_ARG for a grid that breaks a rule of its struct or a null output. */
int rt_probe_positions_device(const rt_probe_grid* grid, const double* d_offsets, rt_surfel* d_probes_out, void* stream);
/* Its host twin: host only, no device. */
int rt_debug_probe_positions(const rt_probe_grid* grid, const double* offsets, rt_surfel* probes_out);
/* One step over every probe of the grid: d_offsets (n_probes x 3 doubles) is read and written, d_info (n_probes
   records) is written; neither may be NULL. */
int rt_relocate_probes_device(rt_scene* scene, const rt_probe_grid* grid, const rt_probe_relocate_params* params,
                              int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base,
                              double* d_offsets, rt_probe_relocation* d_info, void* stream);
/* The fold and the rule on the host, no device: rays and hits are n_probes * spp of each, probe i's at
   [i * spp, (i + 1) * spp); offsets in/out, info written.  RT_ERR_ARG as above, and for a null rays or hits. */
int rt_debug_probe_relocate(const rt_probe_grid* grid, const rt_probe_relocate_params* params, const rt_ray* rays,
                            const rt_hit* hits, int32_t spp, double* offsets, rt_probe_relocation* info);
int rt_shade_probes_placed_device(rt_scene* scene, const rt_probe_grid* grid, const double* d_offsets,
                                  const uint32_t* d_state, const double* d_L, const rt_surfel* d_points, int64_t n,
                                  rt_color* d_irradiance, double* d_weight, void* stream);
int rt_shade_probes_placed(rt_scene* scene, const rt_probe_grid* grid, const double* offsets, const uint32_t* state,
                           const double* L, const rt_surfel* points, int64_t n, rt_color* irradiance, double* weight);
int rt_debug_probe_segments_placed_device(const rt_probe_grid* grid, const double* d_offsets, const uint32_t* d_state,
                                          const rt_surfel* d_points, int64_t n, rt_ray* d_rays_out, double* d_t_max_out,
                                          void* stream);
int rt_debug_probe_segments_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state,
                                   const rt_surfel* points, int64_t n, rt_ray* rays_out, double* t_max_out);
int rt_debug_shade_probes_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state, const double* L,
                                 const rt_surfel* points, int64_t n, const uint8_t* occluded, rt_color* irradiance,
                                 double* weight);
int rt_shade_probes_depth_placed_device(const rt_probe_grid* grid, const double* d_offsets, const uint32_t* d_state,
                                        const rt_probe_depth_params* params, const double* d_L, const double* d_D,
                                        const rt_surfel* d_points, int64_t n, rt_color* d_irradiance, double* d_weight,
                                        void* stream);
int rt_debug_shade_probes_depth_placed(const rt_probe_grid* grid, const double* offsets, const uint32_t* state,
                                       const rt_probe_depth_params* params, const double* L, const double* D,
                                       const rt_surfel* points, int64_t n, rt_color* irradiance, double* weight);

/*
 * Obscurance at surfels: occlusion that fades with distance, the bent normal, and the loop that adapts the
 * sample count.  rt_occluded_surfels counts a point's blocked sample segments with an any-hit query; here each
 * sample takes the closest hit, so that a hit weighs by how near it is, and the directions are kept: per entry
 * the sum of the weights (ambient obscurance), of their squares (the variance a stopping rule needs) and of the
 * unoccluded directions (the bent normal).  Plain counts stay the cheap path: rt_occluded_surfels moves 4 B per
 * point and stops at the first hit; this entry traces to the closest hit and moves 112 B per sample through
 * per-scene scratch.
 *
 * Everything below is normative and fp64 as "probe grids" is: every operation rounded on its own, nothing
 * contracted, IEEE division and square root, no library function.
 *
 * The ray.  Sample k of entry e is the ray rt_debug_surfel_rays_device reports for sample k of record e in
 *   gather_mode with (seed, stream_base + e, sample_base + k).  It is keyed by the entry number, not by the list
 *   position.
 * The hit.  Its hit is what rt_query_rays_device(RT_QUERY_FAST) answers for that ray on this scene in its
 *   traversal mode (BRUTE, GROUPED, or BVH with either builder).
 * The accumulation, per entry, samples ascending k = 0 .. spp - 1, into what the record already holds:
 *   a ray whose direction is all zeros (an invalid surfel):  samples += 1, nothing else.  Every listed entry
 *     below n_records therefore gets exactly samples += spp, as rt_occluded_surfels promises;
 *   else  in = prim_id >= 0 and distance < radius  (a NaN distance is not in);  samples += 1;
 *     not in:  w = 0;
 *     in:  hits += 1;  power == 0:  w = 1;  else  x = distance / radius,  b = 1 - x held to [0, 1]
 *          (b < 0 gives 0, b > 1 gives 1),  w = b multiplied by b another power - 1 times, left to right;
 *     o += w;   o2 += w * w;   v = 1 - w;   bent[a] += v * d[a] for a = x, y, z,   each product rounded, then each
 *     sum.  d is the reported ray's direction, a widened fp32.
 * What is promised:
 *   1. The device result equals rt_debug_obscurance_fold over the reported rays and the query's answers, bit for
 *      bit.
 *   2. An entry's result depends on (seed, stream_base + e, the sample indices, the record, the params, the
 *      traversal mode) only: not on n, on n_records, on the entry's place in the list, on chunking or on the
 *      stream.
 *   3. A call of a + b samples equals a call of a samples followed by one of b samples at sample_base + a into
 *      the same array, bit for bit.
 * The list: rt_occluded_surfels_device's rules.  d_index[j], j < n, names the entries; NULL is the identity and
 *   n must equal n_records.  An entry >= n_records is skipped and nothing is written for it; an entry named
 *   twice is undefined.  d_surfels and d_acc have n_records elements.
 * Calls.  `params` is a host pointer.  RT_ERR_ARG, before anything is launched, in rt_occluded_surfels_device's
 *   order: an unknown gather_mode (checked first), a null scene, n < 0, spp <= 0; then, for n > 0, a null
 *   surfels, params or accumulator pointer, n_records <= 0 or >= 2^32, a null index with n != n_records, params
 *   that break a rule of the struct, spp > 2^19 (split the call by sample_base).  RT_ERR_STATE on a BVH2 scene.
 *   n == 0 returns RT_OK and touches nothing.  Always the generic kernels; no camera is needed; the counters of
 *   rt_scene_get_stats, an armed rt_debug_ray_log, the rt_kernel_times ring and the scene-specialised kernels
 *   are left as they were.  Asynchronous on `stream`, ordered like the device-resident renders (the per-scene
 *   scratch rule of the preamble); chunks of max(1, 2^19 / spp) whole list positions (RTCORE_QUERY_CHUNK
 *   samples), 64 + 48 B of per-scene scratch per sample.
 *
 * The rule (rt_obscurance_select_device).  N = samples, n = (double)N.  active(entry), in this order:
 *   1. N < min_samples: 1.     2. N >= max_samples: 0.     3. N < 2: 1.
 *   4. u = o2 - (o * o) / n,  d = u / (n - 1.0);  d a NaN: 0.
 *   5. v = u > (n * 2^-49) * o2 ? d : 0;  se = sqrt(v / n);  active when se > tol.
 *   tol is absolute: obscurance lies in [0, 1].  With power == 0 the weights are 0 or 1 and se is the binomial
 *   standard error sqrt(p (1 - p) / (N - 1)).  The guard of step 5 is "adaptive light probes"': u carries up to
 *   (3 n + 13) 2^-53 o2 of rounding, n 2^-49 o2 is above that for every n, and a difference not above it is
 *   rounding, not variance.  An entry whose samples all weigh the same therefore has se == 0 exactly and stops
 *   at min_samples: open sky, an invalid surfel, the centre of a sphere.
 *   The list is ascending; *d_count is the number of active entries, also when it exceeds cap.  The pass runs on
 *   the calling thread's current device, asynchronous on `stream`.  RT_ERR_ARG for a null pointer (d_list may be
 *   NULL with cap == 0), tol NaN or negative, n_records <= 0 or >= 2^32.  rt_debug_obscurance_select is its host
 *   twin and returns the count (or a negative status).  rt_debug_obscurance_error reports se and mean = o / n as
 *   step 5 reads them; both a quiet NaN where N < 2.
 * Not part of it: a host-buffer entry, a per-entry radius, RT_QUERY_EXACT, fusing the fold into the query
 *   kernel, and any promised relation to rt_occluded_surfels' counts (one-sided culling and ties at the radius
 *   make a few samples differ).
 */
typedef struct rt_obscurance_params {   /* 24 B */
    double   radius;      /* finite, > 0: a hit at this distance or beyond does not obscure */
    int32_t  power;       /* 0 .. 8: 0 counts every hit inside the radius as 1; p >= 1: (1 - d / radius)^p */
    uint32_t reserved[3]; /* 0 */
} rt_obscurance_params;
typedef struct rt_obscurance {          /* 48 B per entry, three 16-byte rows; added to */
    double   o, o2;       /* sum of the samples' weights, and of their squares                 */
    double   bent[3];     /* sum of (1 - weight) * direction: the unnormalised bent normal     */
    uint32_t samples;     /* samples taken (an invalid surfel's count too)                     */
    uint32_t hits;        /* samples with a hit inside the radius                              */
} rt_obscurance;
typedef struct rt_obscurance_select_params {   /* 16 B */
    double   tol;          /* >= 0, not NaN: converged when se <= tol (absolute: obscurance lies in [0, 1]) */
    uint32_t min_samples, max_samples;
} rt_obscurance_select_params;
int rt_obscurance_surfels_device(rt_scene* scene, int32_t gather_mode, const rt_surfel* d_surfels, int64_t n_records,
                                 const uint32_t* d_index, int64_t n, const rt_obscurance_params* params, int32_t spp,
                                 uint64_t seed, uint64_t sample_base, uint64_t stream_base, rt_obscurance* d_acc,
                                 void* stream);
/* Its fold on the host, no device: rays and hits are n * spp of each, entry i's at [i * spp, (i + 1) * spp). */
int rt_debug_obscurance_fold(const rt_obscurance_params* params, const rt_ray* rays, const rt_hit* hits, int64_t n,
                             int32_t spp, rt_obscurance* acc);
int rt_obscurance_select_device(const rt_obscurance_select_params* params, const rt_obscurance* d_acc, int64_t n_records,
                                uint32_t* d_list, uint32_t cap, uint32_t* d_count, void* stream);
int64_t rt_debug_obscurance_select(const rt_obscurance_select_params* params, const rt_obscurance* acc, int64_t n_records,
                                   uint32_t* list, uint32_t cap);
int rt_debug_obscurance_error(const rt_obscurance_select_params* params, const rt_obscurance* acc, int64_t n,
                              double* se_out, double* mean_out);

/* ---------------------------------------------------- indexed radiance queries --- */
/*
 * rt_render_list / rt_render_list_device: rt_render_rays, rt_render_beams or rt_render_surfels for a list
 * of entry numbers into an array of records, added into accumulators indexed by entry, optionally with
 * the moments of "adaptive sampling" below -- what rt_render_pixels is to a frame.  A caller that wants
 * more samples of some entries only lists those: nothing is compacted, and no entry's stream changes.
 * With rt_adaptive_select_device over the per-entry accumulators (a "frame" of n_records pixels) a
 * lightmap, a probe grid or a panorama of the host's own is rendered until its error is below a bound.
 *
 * Records.  records holds n_records records of the type `kind` names: rt_ray, rt_beam or rt_surfel.
 * gather_mode is the surfels' rt_gather_mode and must be 0 for rays and beams.
 * The list.  index holds n entry numbers e = index[j]; index == NULL is the identity list, and n must
 * then equal n_records.
 * Sampling (normative).  Sample k of entry e is the sample the kind's own entry point defines for record
 * e of the array: it draws from rt_rng_init(seed, stream_base + e, sample_base + k).  The stream is keyed
 * by the entry number, not by the list position j.
 * Accumulation.  Everything is added at index e.  sum, samples, misses and the ray count follow
 * rt_render_rays' rule (a primary miss is counted in misses and not added to sum).
 * Moments.  q and batches come both or neither, else RT_ERR_ARG, and follow rt_render_pixels' rule word
 * for word: every work item j of an entry with t_j = samples + misses > 0 finished samples is one batch;
 * Y_j is the fp64 luminance 0.299 r + 0.587 g + 0.114 b of the item's fp32 colour sums, left to right,
 * each operation rounded on its own, a miss counting as luminance 0;
 *     q[e] += sum over the call's batches of Y_j * Y_j / t_j            batches[e] += their number
 * (the call's terms are summed in item order and added to q once).
 * The estimate is that of "adaptive sampling": N = samples + misses, Y = 0.299 sum.r + 0.587 sum.g +
 * 0.114 sum.b, J = batches, Q = q, s2 = max(0, (Q - Y * Y / N) / (J - 1)) for J >= 2 and se = sqrt(s2 / N),
 * the standard error of the entry's mean luminance, and rt_adaptive_select_device's rule applies as it
 * stands.  Its limit: it is the error of sum / N, misses counted as black.  For a gather that is the
 * gathered mean (sum + misses * ambient) / N only where the ambient colour is black or the entry has no
 * misses; elsewhere the misses' constant ambient term is counted as if it varied, and se over-estimates.
 *
 * What is promised (normative):
 *   1. With index == NULL, plane == 0 and no moments, from equal accumulator contents, the result is
 *      rt_render_rays_device's, rt_render_beams_device's or rt_render_surfels_device's bit for bit (and
 *      rt_render_list's the host entries').
 *   2. An entry's five accumulators depend on (seed, stream_base + e, the sample indices, the record, the
 *      traversal mode) only: not on n, on n_records, on the entry's place in the list, on the host entry's
 *      chunking or on the stream.  The samples per work item are s = min(64, ceil(spp / B)), B = 24 (BRUTE,
 *      GROUPED) or 64 (BVH), a function of spp alone.
 *   3. Coherence: entries 64 j .. 64 j + 63 of the list share a wave for every sample, so list neighbouring
 *      records next to each other; rt_adaptive_select_device's block order over a texel grid does.
 *
 * rt_render_list_device: d_records resident on the scene's device; accumulators of n_records elements,
 * the sum as planes R | G | B `plane` elements apart (0 = n_records).  Asynchronous on `stream`, ordered
 * like the device-resident renders; one launch, RT_ERR_ARG for n above rt_render_rays_device's bound at
 * this spp.  An entry >= n_records is skipped: not traced, nothing written.  An entry named twice is
 * undefined (its accumulators are updated by two threads).
 * rt_render_list (host): caller arrays of n_records elements (sum_rgb one rt_color per entry, as
 * rt_render_rays), everything added to, every entry not in the list untouched.  Synchronous, on the
 * scene's own stream; any n, in rt_render_rays' chunks (2^19 entries, 2^18 for beams; RTCORE_QUERY_CHUNK;
 * fewer where spp makes a chunk's items pass 2^26), two of them resident, copies overlapping the kernels:
 * the listed records and 4 B up, one 48-B record down per entry.  RT_ERR_ARG also for an entry >=
 * n_records and for an entry named twice (checked with a bitmap before anything is launched).
 *
 * Errors, before anything is launched: RT_ERR_ARG for an unknown kind (checked first), then an unknown
 * gather_mode (surfels) or a non-zero one (rays, beams), a null scene, n < 0, spp <= 0, only one of q /
 * batches; then, for n > 0, a null records, sum, samples or misses pointer, n_records <= 0, n_records >=
 * 2^32, plane non-zero and below n_records, a null index with n != n_records.  RT_ERR_STATE on a BVH2
 * scene.  n == 0 (with arguments that pass the first group) returns RT_OK and touches nothing.  No camera
 * is needed.  Always the generic kernels; the counters of rt_scene_get_stats, an armed rt_debug_ray_log,
 * rt_kernel_times and the scene-specialised kernels are left as they were.
 */
typedef enum rt_list_kind { RT_LIST_RAYS = 0, RT_LIST_BEAMS = 1, RT_LIST_SURFELS = 2 } rt_list_kind;
int rt_render_list_device(rt_scene* scene, int32_t kind, int32_t gather_mode, const void* d_records, int64_t n_records,
                          const uint32_t* d_index, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                          uint64_t stream_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses, double* d_q,
                          uint32_t* d_batches, uint64_t plane, unsigned long long* d_rays_count, void* stream);
int rt_render_list(rt_scene* scene, int32_t kind, int32_t gather_mode, const void* records, int64_t n_records,
                   const uint32_t* index, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base, uint64_t stream_base,
                   rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches,
                   uint64_t* rays_out);

/* ----------------------------------------------------------- adaptive sampling --- */
/*
 * rt_render_pixels / rt_render_pixels_device: spp of the camera's own samples, exactly as a tile render
 * draws them, for a list of frame pixels, added into whole-frame accumulators; optionally two more
 * accumulators from which a per-pixel standard error follows.  rt_adaptive_select_device turns such
 * accumulators into the next pixel list on the device, so a "render until the noise is below x" loop
 * runs without the image leaving device memory.
 *
 * A list entry is the frame pixel index fy * width + fx (the number rt_rng_pixel_key is keyed by).
 * The path kernels run in the scene's traversal mode (BRUTE, GROUPED or BVH with either builder;
 * RT_ERR_STATE on a BVH2 scene, as rt_render_rays), always the generic kernels, whatever rt_set_jit says.
 *
 * What is promised (normative):
 *   - Sample k of a listed pixel is the sample rt_render_tile_1spp(seed, sample_base + k) returns for
 *     it, bit for bit, in the scene's traversal mode: the stream rt_rng_init(seed, pixel, sample_base + k)
 *     with nothing discarded (GetCameraRay's two draws are used, then the depth-of-field and bounce draws).
 *   - A pixel's result depends on (seed, pixel, the sample indices, the traversal mode) only: not on n,
 *     on the pixel's place in the list or on the host entry's chunking.  The samples per work item are
 *     s = min(64, ceil(spp / B)), B = 24 (BRUTE, GROUPED) or 64 (BVH), a function of spp alone; an
 *     item's samples are summed in fp32 in sample order and the items folded into fp64 in sample order.
 *   - The sums equal rt_render_device's bit for bit from equal accumulator contents wherever that
 *     launch puts the same samples into an item: any window of at most 1920 x 1080 pixels at spp <= B,
 *     and a window of exactly 2,073,600 pixels at any spp.
 *   - rays_out / d_rays count the Scene.RayTrace equivalents in rt_render_tile's unit (added to).
 *   - Coherence: entries 64 j .. 64 j + 63 share a wave for every sample, so list neighbouring pixels
 *     next to each other; rt_adaptive_select_device's order does.
 *
 * The moments.  With q and batches (both or neither, else RT_ERR_ARG) every work item j of a pixel with
 * t_j = samples + misses > 0 finished samples is one batch: with Y_j = 0.299 r + 0.587 g + 0.114 b of
 * the item's fp32 colour sums (DoubleColor.GetLuminance, DoubleColor.cs:76-79, in fp64, left to right,
 * each operation rounded on its own; a miss counts as luminance 0),
 *     q[pixel] += sum over the call's batches of Y_j * Y_j / t_j        batches[pixel] += their number
 * (the call's terms are summed in item order and added to q once).  The estimate these give:
 *     N = samples + misses,  Y = 0.299 sum.r + 0.587 sum.g + 0.114 sum.b,  J = batches,  Q = q
 *     variance per sample  s2 = max(0, (Q - Y * Y / N) / (J - 1))    for J >= 2
 *     standard error of the pixel's mean luminance  se = sqrt(s2 / N)
 * Batches of unequal size keep it unbiased: E[sum Y_j^2 / t_j] - E[Y^2 / N] = (J - 1) s2.  Up to spp = B
 * per call every batch is one sample and s2 is the plain sample variance.  It adds over calls, over
 * sample_base ranges and over GPUs.
 *
 * rt_render_pixels (host): whole-frame caller buffers in the x * height + y order, everything added to,
 * every pixel not in the list untouched (rt_render_bands' contract with a list in the band set's
 * place).  q and batches may both be NULL.  Synchronous, on the scene's own stream; any n, in chunks of
 * at most 2^19 entries (RTCORE_QUERY_CHUNK; fewer where spp makes a chunk's items pass 2^26), two of
 * them resident, uploads and downloads overlapping the kernels as in rt_render_rays: 4 B up and one
 * 48-B record down per entry.  RT_ERR_ARG also for an entry >= width * height and for a pixel named twice
 * (checked with a bitmap of the frame before anything is launched).
 * rt_render_pixels_device: accumulators in rt_render_device's layout over the whole frame, index
 * y * width + x, planes `plane` elements apart (0 = width * height).  Asynchronous on `stream`, ordered
 * like the device-resident renders; one launch, RT_ERR_ARG for n above rt_render_rays_device's bound at
 * this spp.  An entry outside the frame is skipped: not traced, nothing written.  A pixel named twice
 * is undefined (its accumulators are updated by two threads).
 *
 * Errors, before anything is launched: RT_ERR_ARG for a null scene, a null list or sum, samples or
 * misses pointer, only one of q / batches, n < 0, spp <= 0, a frame of 2^32 pixels or more or of more
 * than 2^20 rows; RT_ERR_STATE without a camera and on a BVH2 scene.  n == 0 returns RT_OK and touches
 * nothing.  The counters of rt_scene_get_stats, an armed rt_debug_ray_log, rt_kernel_times and the
 * scene-specialised kernels are left as they were.
 */
int rt_render_pixels(rt_scene* scene, const uint32_t* pixels, int64_t n, int32_t spp, uint64_t seed, uint64_t sample_base,
                     rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, double* q, uint32_t* batches,
                     uint64_t* rays_out);
int rt_render_pixels_device(rt_scene* scene, const uint32_t* d_pixels, int64_t n, int32_t spp, uint64_t seed,
                            uint64_t sample_base, double* d_sum, uint32_t* d_samples, uint32_t* d_misses, double* d_q,
                            uint32_t* d_batches, uint64_t plane, unsigned long long* d_rays, void* stream);

/*
 * The selection rule.  With N, Y, Q, J of a pixel as above, active(N, Y, Q, J) is, in this order:
 *   1. N < min_samples   -> 1
 *   2. N >= max_samples  -> 0
 *   3. J < 2             -> 1
 *   4. otherwise  se > rel_tol * max(Y / N, lum_floor)
 * A NaN in an accumulator makes step 4's comparison false: the pixel is inactive (it cannot converge,
 * so it is not sampled for ever).  An all-miss pixel (Y = Q = 0) has se = 0 and stops at min_samples.
 */
typedef struct rt_adaptive_params {   /* 32 B */
    double   rel_tol;      /* converged when se <= rel_tol * max(Y / N, lum_floor)          */
    double   lum_floor;    /* > 0; keeps black pixels from never converging                 */
    uint32_t min_samples;  /* a pixel with N < min_samples is always active                 */
    uint32_t max_samples;  /* a pixel with N >= max_samples is never active                 */
    uint32_t reserved[2];  /* 0 */
} rt_adaptive_params;
/*
 * rt_adaptive_select_device: the active pixels' frame indices into d_pixels, from accumulators in
 * rt_render_pixels_device's layout (planes `plane` apart, 0 = width * height), on the calling thread's
 * current device (as rt_tonemap_device), asynchronous on `stream`.  The order is normative: by 8 x 8
 * block of the frame, blocks row-major; within a block by (y & 7) * 8 + (x & 7), the path kernels' own
 * pixel order, so 64 consecutive entries are a few neighbouring blocks.  *d_count receives the number
 * of active pixels, also when it exceeds cap; then only the first cap are stored.  Deterministic: a
 * count per block (one wave per block, ballot), an exclusive scan over the block counts, the write
 * by ballot prefix; no atomic decides a position.  The temporary block counts are the library's own,
 * per device; calls on one device are serialised by the caller.  RT_ERR_ARG for a null pointer (d_pixels
 * may be NULL with cap = 0), rel_tol or lum_floor NaN or negative, lum_floor == 0, a frame of no pixels
 * or of 2^32 or more.
 * rt_debug_adaptive_select: the host twin (host only, no device needed): the same arguments on host
 * arrays in the same layout, the same rule function, the same order; returns the count (at most cap
 * entries stored), or a negative rt_status.
 */
int rt_adaptive_select_device(const rt_adaptive_params* params, const double* d_sum, const uint32_t* d_samples,
                              const uint32_t* d_misses, const double* d_q, const uint32_t* d_batches, uint64_t plane,
                              int32_t width, int32_t height, uint32_t* d_pixels, uint32_t cap, uint32_t* d_count,
                              void* stream);
int64_t rt_debug_adaptive_select(const rt_adaptive_params* params, const double* sum, const uint32_t* samples,
                                 const uint32_t* misses, const double* q, const uint32_t* batches, uint64_t plane,
                                 int32_t width, int32_t height, uint32_t* pixels, uint32_t cap);

/* ------------------------------------------------------------------- denoising --- */
/*
 * The guide pass.  d_hits[y*w + x] is, bit for bit, what rt_query_rays(RT_QUERY_FAST) answers for the ray
 * rt_camera_rays gives for pixel (x0 + x, y0 + y) of the scene's frame: Camera.GetRay(x, y).Offset(imagePlane),
 * the pixel centre, no lens sample.  The rays are made on the device, in chunks of whole rows of at most
 * 2^19 rays (one row where a row is longer), so the scene's scratch for them stays below rt_query_rays'.
 * Asynchronous on `stream`, ordered like the device-resident renders.  RT_ERR_STATE without a camera and on
 * a BVH2 scene; RT_ERR_ARG for a null pointer, w or h <= 0 or a tile outside the frame.  The generic
 * kernels run, whatever rt_set_jit says; the counters of rt_scene_get_stats, an armed rt_debug_ray_log,
 * rt_kernel_times and the scene-specialised kernels are left as they were.
 */
int rt_primary_hits_device(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h, rt_hit* d_hits, void* stream);

/*
 * rt_denoise_device: an edge-avoiding a-trous filter (the spatial half of SVGF) over whole-frame
 * accumulators with moments, guided by the first hits of rt_primary_hits_device and by the pixels' own
 * variance estimate.  The definition is normative; the device pass and the host twin rt_debug_denoise
 * compile it from one set of functions and agree bit for bit.  Every operation is rounded on its own (no
 * contraction), division and square root are IEEE on both sides, no library function is called.  The
 * state is fp32 unless stated.
 *
 * Valid pixel: samples > 0, the hit's prim_id >= 0, and c and v (below, as fp32) finite.  An invalid
 * pixel passes through -- out_sum = sum bit for bit, out_var = 0 -- and contributes to no other pixel.
 *
 * Preparation, in fp64, each result rounded to fp32 once: c = sum / samples per channel; with N, Y, Q, J
 * and s2 of "adaptive sampling" above, v = s2 * N / samples^2 for J >= 2 (the variance of c's luminance)
 * and v = (Y / samples)^2 for J < 2 (no estimate: the pixel's own luminance squared, which keeps the
 * luminance edge stop wide open).  Guides: the hit's normal n and position x, and d = (float)distance.
 *
 * Level k = 0 .. iterations - 1, step s = 2^k, for a valid pixel p.  Its taps are q = p + s (i, j),
 * i, j in -2 .. 2, inside the frame and valid, visited with j ascending, then i ascending; h = {1/16, 1/4,
 * 3/8, 1/4, 1/16}; the weight of a tap is w = h(i) h(j) w_n w_z w_l, multiplied left to right, and a tap
 * whose w is not above 0 contributes nothing.  The centre tap's w is the constant 9/64, not computed
 * (a centre whose normal is NaN, rt_debug_ray.normal's quirk, keeps its own colour).
 *   w_n = max(0, n_p . n_q)^(2^normal_pow_log2), by that many squarings; a NaN dot product gives 0;
 *         with RT_DENOISE_SAME_PRIM, 0 for a tap of another prim_id
 *   w_z = f(|n_p . (x_q - x_p)| / (sigma_z d_p))               (dot products left to right)
 *   w_l = f(|L(c_q) - L(c_p)| / (sigma_l sqrt(g_p) + lum_eps)),   L = 0.299 r + 0.587 g + 0.114 b
 *   f(t) = 1 / (1 + t + 0.5 t t) for t >= 0, else 0 (NaN gives 0)
 *   g_p = sum k_q v_q / sum k_q over p and its neighbours q = p + (i, j), i, j in -1 .. 1 (distance 1 at
 *         every level), k = {1/4, 1/2, 1/4}^2, that lie in the frame, are valid and have w_n > 0 towards p,
 *         in the same order.  (The w_n > 0 condition keeps the filter from leaking across an edge that
 *         the normals or prim_ids stop: without it a pixel beside the edge would read the variance of the
 *         pixels behind it.)
 *   c' = c_p + sum w (c_q - c_p) / sum w per channel -- an exactly constant image maps to itself --
 *   v' = sum w w v_q / (sum w)^2; the levels ping-pong between two state buffers.
 * Output: out_sum = (double)c * (double)samples per channel and out_var = v after the last level, so
 * rt_tonemap_device(d_out_sum, d_samples, d_misses, ...) works unchanged.
 *
 * Accumulators in rt_render_pixels_device's layout (index y * width + x, planes `plane` elements apart,
 * 0 = width * height); d_hits is rt_primary_hits_device's output for the whole frame; d_out_sum has
 * d_sum's layout and must not overlap it; d_out_var (width * height floats) may be NULL.  The pass runs
 * on the calling thread's current device, asynchronous on `stream`; its scratch (a 32-byte guide record
 * and two 16-byte state records per pixel) is the library's own, per device, grown on demand; a call on
 * another stream than the last one on that device is ordered after it.
 * RT_ERR_ARG, before anything is launched, for a null pointer (d_out_var excepted), a frame of no pixels
 * or of 2^32 or more, out_sum overlapping sum, a sigma or lum_eps that is not above 0 (NaN included),
 * normal_pow_log2 outside 0 .. 8, iterations outside 1 .. 5, unknown flag bits or non-zero reserved.
 * rt_debug_denoise: the host twin (host only, no device needed), the same arguments on host arrays.
 */
#define RT_DENOISE_SAME_PRIM 1u
typedef struct rt_denoise_params {   /* 32 B */
    float    sigma_l;          /* luminance edge stop, in standard deviations; > 0            */
    float    sigma_z;          /* plane-distance edge stop, relative to the centre's distance; > 0 */
    float    lum_eps;          /* > 0, added to sigma_l * sqrt(g) */
    int32_t  normal_pow_log2;  /* 0..8: w_n = max(0, n_p . n_q)^(2^m), by m squarings          */
    int32_t  iterations;       /* 1..5 levels, step 2^k                                        */
    uint32_t flags;            /* RT_DENOISE_SAME_PRIM = 1: a tap of another prim_id weighs 0  */
    uint32_t reserved[2];      /* 0 */
} rt_denoise_params;
int rt_denoise_device(const rt_denoise_params* params, const double* d_sum, const uint32_t* d_samples,
                      const uint32_t* d_misses, const double* d_q, const uint32_t* d_batches, uint64_t plane,
                      const rt_hit* d_hits, int32_t width, int32_t height, double* d_out_sum, float* d_out_var,
                      void* stream);
int rt_debug_denoise(const rt_denoise_params* params, const double* sum, const uint32_t* samples,
                     const uint32_t* misses, const double* q, const uint32_t* batches, uint64_t plane,
                     const rt_hit* hits, int32_t width, int32_t height, double* out_sum, float* out_var);

/* ------------------------------------------------------- temporal reprojection --- */
/*
 * rt_reproject_device: carries whole-frame accumulators with moments from the pixels of a previous camera
 * to the pixels of the scene's current one (the temporal half of SVGF's history, for a static scene and a
 * moving camera), so that an adaptive render continues from them instead of from zero.  A nearest-pixel
 * gather: each current pixel takes the five accumulators of at most one previous pixel, so (Y, N, Q, J)
 * stays the sample set of one pixel and the estimate of "adaptive sampling" keeps its meaning; mixing the
 * moments of several pixels would not.  The definition is normative; the device pass and the host twin
 * rt_debug_reproject compile it from one set of functions and agree bit for bit.  Every operation is
 * rounded on its own (no contraction), division is IEEE on both sides, no library function is called on
 * the device.
 *
 * The host runs Camera.InitRender on prev_camera for (width, height) once -- position, look, side, up, w2,
 * h2, tan_x, tan_y, h_mult, v_mult in fp64, as the exact kernels hold them -- and hands the result to the
 * pass.  For the current pixel p = (x, y) with H = d_hits[y * width + x]:
 *  1. Invalid: H.prim_id < 0 or a component of H.position not finite -- p is empty (6).
 *  2. Projection, in fp64: X = H.position widened, v = X - position, z = v . look, a = v . side, b = v . up
 *     (dot products left to right).  Empty unless z > 0.
 *       frustum: fx = w2 + w2 * ((a / z) / tan_x),  fy = h2 + h2 * ((b / z) / tan_y)
 *       ortho:   fx = w2 + a / h_mult,              fy = h2 + b / v_mult
 *     the inverse of FrustumCamera.GetRay (offX = tanFOVX2 * ((x - w2) / w2)) and OrthoCamera.GetRay.  Pixel
 *     centres are the integer coordinates (rt_camera_rays traces GetRay(x, y)).  Empty unless
 *     fx >= -0.5 && fx < width - 0.5 && fy >= -0.5 && fy < height - 0.5 (a NaN fails).  qx = (int)(fx + 0.5),
 *     qy = (int)(fy + 0.5), a floor here; held to width - 1 and height - 1 (only a frame one pixel wide
 *     or high can reach them, by the sum's rounding).
 *  3. Validation against G = d_prev_hits[qy * width + qx]; p is empty unless all of
 *       G.prim_id >= 0;  with RT_REPROJECT_SAME_PRIM, G.prim_id == H.prim_id;  G.inside == H.inside;
 *       n_H . n_G >= normal_cos_min                                  (fp32, left to right; a NaN rejects)
 *       |n_H . (x_G - x_H)| <= sigma_z * (float)H.distance           (fp32, as rt_denoise_device's w_z: the
 *                                                                     differences first; a NaN rejects)
 *  4. History: N = samples + misses of the source pixel (64-bit).  Empty if N == 0.  If N <= max_history
 *     the five accumulators are copied bit for bit.
 *  5. The cap, N > max_history: N' = max_history, samples' = (uint32)((uint64)samples * N' / N), misses' =
 *     N' - samples'; per channel sum' = sum * ((double)samples' / (double)samples) for samples > 0, else
 *     sum; with Y, Y' the luminances of sum, sum' (0.299 r + 0.587 g + 0.114 b, fp64, left to right):
 *       J >= 2: J' = min(J, N'), D = Q - Y * Y / N, Q' = D * ((double)(J' - 1) / (double)(J - 1)) + Y' * Y' / N'
 *       J <  2: J' = J, Q' = Q * ((double)N' / (double)N)
 *     The mean colour sum / samples is kept to rounding and the per-sample variance s2 by construction,
 *     (Q' - Y'^2 / N') / (J' - 1) = D / (J - 1); only the history's weight drops, so that samples of the
 *     new view outvote it and view-dependent shading recovers.
 *  6. An empty pixel gets 0 in all five accumulators and out_src = -1; an accepted one out_src =
 *     qy * width + qx.
 * Miss pixels are not reprojected.  A depth-of-field camera is accepted: the hits are the pinhole
 * centre's, so the history is that footprint's.
 *
 * d_prev_hits is rt_primary_hits_device's whole-frame output under prev_camera, d_hits the same under the
 * current camera; the pass itself needs no scene.  Inputs and outputs in rt_render_pixels_device's layout
 * (index y * width + x, sum planes `plane` elements apart, 0 = width * height); d_out_src (width * height
 * int32) may be NULL.  No output may overlap an input: the pass is a gather, an overlap would be a race.
 * Runs on the calling thread's current device, asynchronous on `stream`; no scratch memory.
 * RT_ERR_ARG, before anything is launched, for a null pointer (d_out_src excepted), a frame of no pixels
 * or of 2^32 or more, a plane smaller than the frame, d_out_sum overlapping d_sum, an unknown camera kind,
 * sigma_z not above 0 (NaN included), normal_cos_min outside [-1, 1] or NaN, max_history == 0, unknown
 * flag bits or non-zero reserved fields.
 * rt_debug_reproject: the host twin (host only, no device needed), the same arguments on host arrays.
 */
#define RT_REPROJECT_SAME_PRIM 1u
typedef struct rt_reproject_params {   /* 32 B */
    float    sigma_z;         /* > 0: plane-distance stop, relative to the current hit's distance */
    float    normal_cos_min;  /* in [-1, 1]: the two normals' dot product must be >= this          */
    uint32_t max_history;     /* >= 1: a carried pixel has at most this many samples + misses      */
    uint32_t flags;           /* RT_REPROJECT_SAME_PRIM: the source must show the same prim_id     */
    uint32_t reserved[4];     /* 0 */
} rt_reproject_params;
int rt_reproject_device(const rt_reproject_params* params, const rt_camera* prev_camera,
                        const rt_hit* d_prev_hits, const rt_hit* d_hits,
                        const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses,
                        const double* d_q, const uint32_t* d_batches, uint64_t plane,
                        int32_t width, int32_t height,
                        double* d_out_sum, uint32_t* d_out_samples, uint32_t* d_out_misses,
                        double* d_out_q, uint32_t* d_out_batches, int32_t* d_out_src, void* stream);
int rt_debug_reproject(const rt_reproject_params* params, const rt_camera* prev_camera,
                       const rt_hit* prev_hits, const rt_hit* hits,
                       const double* sum, const uint32_t* samples, const uint32_t* misses,
                       const double* q, const uint32_t* batches, uint64_t plane,
                       int32_t width, int32_t height,
                       double* out_sum, uint32_t* out_samples, uint32_t* out_misses,
                       double* out_q, uint32_t* out_batches, int32_t* out_src);

/* Device-side DebugRaycaster Primitives pass: d_ids[y*w + x].  Asynchronous. */
int rt_primary_ids_device(rt_scene* scene, int32_t x0, int32_t y0, int32_t w, int32_t h,
                          int32_t* d_ids, void* stream);

/* Duration in ms of the last path-tracing kernel launched on this scene (hipEvent pair).
 * Waits for that kernel.  RT_ERR_ARG before the first launch. */
int rt_last_kernel_ms(rt_scene* scene, float* ms);

/* Durations in ms of the last n path-tracing kernels launched on this scene, oldest first
 * (1 <= n <= 64 and n <= the launches so far, else RT_ERR_ARG).  Each launch records its own
 * event pair in a ring of 64, so a caller can queue up to 64 launches without a host sync and
 * read their times afterwards.  Waits for those kernels.
 * A time is the time the launch had to itself: t_end[k] - max(t_start[k], t_end[k - 1]), k - 1 the
 * launch recorded before it.  rt_render_device and rt_render_bands_device run consecutive launches on
 * two internal streams, so that a launch's path kernel begins in the SIMDs the one before it is leaving
 * (launch overlap; RTCORE_LAUNCH_OVERLAP=0 turns it off): its start event fires
 * while its predecessor still runs, and the raw pair would count that time twice.  For a launch that
 * began after its predecessor ended, this is the raw event pair.  The times of n consecutive launches
 * add up to no more than the time from the first one's start to the last one's end. */
int rt_kernel_times(rt_scene* scene, int32_t n, float* ms);
/* The same n entries as their raw event pairs, t_end[k] - t_start[k]: what rt_kernel_times returned before
 * launch overlap, and still returns for a launch that began after its predecessor ended (a debug entry:
 * tests compare the two). */
int rt_debug_kernel_times_raw(rt_scene* scene, int32_t n, float* ms);

/*
 * Instrumentation (profiling builds of the measurement, not the render): while enabled, the
 * path kernel's instrumented variant runs and adds up, over all launches since the last read,
 *   [0] BVH node visits  [1] triangle tests  [2] sphere tests           (per ray segment)
 *   [3] wave cycles in work fetch + camera ray  [4] in traversal  [5] in shading
 *   [6] wave loop iterations  [7] BVH kernels: the most traversal steps one query took (max)
 *   [8] wide BVH kernel: traversal-stack entries written past the LDS part (global overflow)
 *   [9] wide BVH kernel: the deepest traversal stack of any lane (max)
 *   [10] BVH kernels: faces of the outer records tested (rectangles and closed boxes' faces left
 *        out of the tree, build statistic [21]; wave-uniform records, not in [1])
 * rt_scene_get_stats synchronises the device, copies min(n, RT_STATS_COUNT) counters and zeroes them.
 */
#define RT_STATS_COUNT 11
int rt_scene_set_stats(rt_scene* scene, int32_t enable);
int rt_scene_get_stats(rt_scene* scene, uint64_t* out, int32_t n);

/* ------------------------------------------------------------- multi-GPU ---- */
/*
 * Row bands.  A band set (band, stride, offset) is the frame rows y with
 * (y / band) % stride == offset.  rt_frame deals the rows of a frame to n devices as the sets
 * (8, n, g), g = 0..n-1: interleaved bands balance background-heavy rows, where the
 * reference's contiguous tiles (FullRaytracer.cs:71-72) would not.
 *
 * rt_render_bands renders one band set on one scene and adds it into whole-frame buffers
 * (x*height + y order, every row outside the set untouched): the per-device step of
 * rt_frame_render, with the same device layout, callable on one device.
 */
int rt_render_bands(rt_scene* scene, int32_t band, int32_t band_stride, int32_t band_offset, int32_t spp,
                    uint64_t seed, uint64_t sample_base, rt_color* sum_rgb, uint32_t* samples,
                    uint32_t* misses, uint64_t* rays_out);

/*
 * Device-resident band-set render for hosts that run one process (or worker) per GPU: adds spp
 * samples of every pixel of the set into planar accumulators, row-major over the set's rows in
 * frame order: d_sum planes R | G | B each `plane` doubles apart, d_samples / d_misses `plane`
 * elements each (plane = 0: rows of the tallest set of the split x width, the gather-slot layout
 * of rt_frame).  Asynchronous on `stream`, like rt_render_device.
 */
int rt_render_bands_device(rt_scene* scene, int32_t band, int32_t band_stride, int32_t band_offset,
                           int32_t spp, uint64_t seed, uint64_t sample_base, double* d_sum,
                           uint32_t* d_samples, uint32_t* d_misses, uint64_t plane,
                           unsigned long long* d_rays, void* stream);
/* Rows of a frame of `height` rows in band set (band, band_stride, band_offset); host only. */
int rt_band_rows(int32_t height, int32_t band, int32_t band_stride, int32_t band_offset);
/* Rows of the tallest band set of the split (band, band_stride, *): a gather slot's plane is
 * this x width (host only). */
int rt_band_slot_rows(int32_t height, int32_t band, int32_t band_stride);
/* Host only: rt_frame_render's merge step for one device's gathered slot -- the slot (Σr | Σg | Σb
 * fp64 planes, then samples and misses u32 planes, each `plane` elements, row-major over the band
 * set's rows in frame order) added into frame buffers in the x*height + y order.  Exposed so that
 * the single-process frame path's band layout can be checked against a per-rank host's (the
 * torch.distributed split of bench.py, raytracercore_amd/sharding.py) without devices. */
int rt_scatter_band_slot(const void* slot, uint64_t plane, int32_t width, int32_t height, int32_t band,
                         int32_t band_stride, int32_t band_offset, rt_color* sum_rgb, uint32_t* samples,
                         uint32_t* misses);

/*
 * Persistent whole-frame renderer over devices 0..n_gpus-1 of this process (replaces the
 * FullRaytracer worker pool, FullRaytracer.cs:297-302, for a multi-GPU host): one scene per
 * device and one RCCL communicator, created once.  Each rt_frame_render call renders spp
 * samples (indices sample_base .. sample_base+spp-1) of every pixel: each device its band set,
 * then one RCCL gather over xGMI to device 0, and adds the result into the caller's frame
 * buffers (x*height + y; SampleSet semantics as rt_render_tile).  Progressive callers pass
 * disjoint sample_base ranges with the same seed.
 */
typedef struct rt_frame rt_frame; /* opaque */
int rt_frame_create(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims,
                    const rt_camera* camera, int32_t n_gpus, rt_frame** out_frame);
int rt_frame_set_camera(rt_frame* frame, const rt_camera* camera);
int rt_frame_render(rt_frame* frame, int32_t spp, uint64_t seed, uint64_t sample_base,
                    rt_color* sum_rgb, uint32_t* samples, uint32_t* misses, uint64_t* rays_out);
/*
 * rt_frame_render in two phases, for a host that keeps the devices busy while it merges: submit
 * queues a render (every device's band set, the RCCL gather to device 0 and the copy of the
 * gathered slots into pinned host memory) and returns at once; collect waits for the oldest
 * submitted render and adds it into the caller's buffers (as rt_frame_render).  At most two
 * renders are in flight (RT_ERR_STATE otherwise), so submit(k+1) before collect(k) overlaps
 * render k+1 with the gather, copy and merge of render k -- FullRaytracer's update loop
 * (FullRaytracer.cs:326-344) merging finished passes while the workers render the next.  No
 * caller buffer is held between calls.  After an error every queued render is dropped.
 */
int rt_frame_submit(rt_frame* frame, int32_t spp, uint64_t seed, uint64_t sample_base);
int rt_frame_collect(rt_frame* frame, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses,
                     uint64_t* rays_out);
/* Test hook: point 1 makes the next gather fail inside its RCCL group (the group is still closed). */
int rt_frame_inject_fault(rt_frame* frame, int32_t point);
void rt_frame_destroy(rt_frame* frame);

/* One-shot rt_frame_create + rt_frame_render + rt_frame_destroy. */
int rt_render_frame_multi(const rt_scene_params* params, const rt_prim* prims, int32_t n_prims,
                          const rt_camera* camera, int32_t n_gpus, int32_t spp, uint64_t seed,
                          uint64_t sample_base, rt_color* sum_rgb, uint32_t* samples, uint32_t* misses,
                          uint64_t* rays_out);

/* ------------------------------------------------------------- scene text ---- */
/*
 * SceneLoader.FromFile restatement (SceneLoader.cs:112-440): parses scene text into
 * primitives (insertion order = Primitive.ID), cameras and scene params.  Two-call
 * protocol: pass NULL arrays to query the counts, then call again with arrays of at
 * least that size.  Returns RT_ERR_PARSE with the line number in rt_last_error().
 */
int rt_parse_scene(const char* text, rt_scene_params* params, rt_prim* prims, int32_t* n_prims,
                   rt_camera* cameras, int32_t* n_cameras);

/*
 * Diagnostic, host only (no device needed): the reference agglomerative BVH the exact pass
 * uses (BVH.cs:193-236), flattened depth-first.  leaf_order[n] receives primitive indices in
 * depth-first leaf order; boxes (may be NULL, room for 2n-1 nodes) receives 8 doubles per node
 * (min xyzw, max xyzw) in pre-order.
 */
int rt_ref_bvh_export(const rt_prim* prims, int32_t n_prims, int32_t* leaf_order, double* boxes,
                      int32_t* n_nodes, int32_t* depth);

/*
 * SampleSet.GetOutput (SampleSet.cs:61-113) on the device, for every pixel of accumulators in
 * rt_render_device's layout (row-major w*h, d_sum planes R | G | B): d_argb[y*w + x] receives the
 * Color.ToArgb code the UI bitmap stores.  Uses the calling thread's current device.  Asynchronous.
 */
int rt_tonemap_device(const double* d_sum, const uint32_t* d_samples, const uint32_t* d_misses, int32_t w, int32_t h,
                      rt_color background, double background_alpha, double exposure, int32_t* d_argb, void* stream);

/* SampleSet.GetOutput (SampleSet.cs:61-113): tonemap accumulators to ARGB. */
int32_t rt_sample_output(rt_color sum, uint32_t samples, uint32_t misses, rt_color background,
                         double background_alpha, double exposure);

#ifdef __cplusplus
}
#endif

#endif /* RTCORE_H */
