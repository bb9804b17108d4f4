// scene_records.h -- the fp32 records of a scene, built on the host only (scene_records.cpp): the
// per-primitive PrimF / TestRec, the brute-force slot orders, materials, transforms, outer records.
#pragma once
#include <vector>

#include "host_scene.h"

namespace rtc {

PrimF make_primf(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, int i);
TestRec make_testrec(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, int i);
float as_f(int v); // the bits of v as a float
float as_f(uint32_t v);
float4 f4(Vec4d v, float w);
// The exact fp64 set (rt_internal.h): one PrimD per primitive ID, one XformD per transformed sphere.
// Shared by the scene upload and the host twin of the selection pass (rt_debug_select_rays).
void make_exact_records(const std::vector<HostPrim>& H, std::vector<PrimD>& pd, std::vector<XformD>& xd);

// The brute-force slot orders of a scene (flat and grouped), built on the host only: world
// rectangles, closed and open boxes, frames, triangles, spheres and planes.
struct BruteLayout {
    int rects = 0, boxes = 0, frames = 0, frame_boxes = 0, frame_rects = 0, tris = 0, sphs = 0;
};
struct BruteOrder {
    std::vector<PrimF> prims;
    std::vector<TestRec> tests;
    std::vector<RectRec> rects;
    std::vector<FrameRec> frames; // FrameRecs and BoxRecs
    std::vector<GroupRec> groups;
    int nr[3] = {0, 0, 0}, nt = 0, ns = 0;
    // a group with more triangles or spheres than GroupRec::n_tri_sph holds (16 and 15 bits): the
    // brute-force kernels cannot run the order (rt_scene_set_traversal refuses them)
    bool overflow = false;
    int tris0 = 0, sphs0 = 0; // triangles and spheres of the first group (the flat order's only one)
};
struct BruteOrders {
    BruteOrder flat, grouped;
    BruteOrder outer; // the BVH's outer records: one group, slots numbered from 0 (planes appended)
    int nr[3] = {0, 0, 0}, nt = 0, ns = 0, np = 0;
    int group_max = 0; // primitives per group of the grouped order (kGroupMax at creation)
    BruteLayout layout;
};
int rect_axis_of(const HostPrim& p); // the plane's axis of an axis-aligned rectangle, or -1

// group_max: primitives per group of the grouped order, which cuts sah (RTCORE_GROUP_MAX overrides it).
// outer: the primitives the BVH leaves out (rt_scene::bvh_outer, may be empty); they get an order
// of their own (BruteOrders::outer), one group of world rects and closed boxes.
BruteOrders make_brute_orders(const std::vector<HostPrim>& H, const std::vector<int>& xf_index, const SahBvh& sah,
                              int group_max, const std::vector<char>& outer = {});

// Everything the record consumers derive from the prepared primitives before they build anything
// else: the transformed spheres' fp32 transforms and their index per primitive, the counts, the
// brute-force orders.
struct HostRecords {
    std::vector<int> xf_index; // per primitive: its XformF, or -1
    std::vector<XformF> xf;
    int n_bvh = 0, n_planes = 0, n_vn = 0; // non-plane primitives, planes, vertex-normal triangles
    int sah_root = 0;                      // root reference of the tree the grouping cut
    BruteOrders orders;
};
// sah: the tree the grouped order cuts; null: built here with leaves of max_leaf primitives
// (max_leaf 0: no tree, so no grouped order).
HostRecords make_host_records(const std::vector<HostPrim>& H, int max_leaf, int group_max, const SahBvh* sah = nullptr,
                              const std::vector<char>* outer = nullptr);

// Leaf size of the SAH tree that the grouped order cuts, per caller.  The callers disagree, and the
// records they make for one scene can differ with them; kept as found, to be settled here.
enum class GroupingTree {
    Scene,        // rt_scene_create (build_bvhs): the tree the kernels traverse too
    LayoutReport, // rt_debug_brute_layout, rt_debug_flat_records
    JitHeader,    // rt_debug_jit_header
};
int grouping_max_leaf(GroupingTree who, int n_prims, bool has_outer);

// Materials, deduplicated: one MatF per distinct record, PrimF.d.w its index.  A 1M-triangle
// mesh of one material then shades from a table of a few records (cache-resident) instead of
// gathering 80 B per hit from an 80 MB per-primitive array.
struct MatTable {
    std::vector<MatF> mats;
    std::vector<int32_t> mat_of; // per primitive ID
};
MatTable make_materials(const std::vector<HostPrim>& H, double air_ior);

std::vector<GroupRec> groups_nearest_first(const std::vector<GroupRec>& g, const CameraD& cam);
XformF make_xformf(const HostPrim& p);
uint32_t scene_facts(const std::vector<HostPrim>& H); // FACT_*
// The padded box over every primitive but the planes, and the origin limit its pad covers.
SceneBound make_scene_bound(const std::vector<HostPrim>& H);
// The flat order's test units (rt_kernels.h, flat_unit_count: world rectangles, world boxes, frames,
// triangle records, sphere records, as trace_brute runs them) and one box per unit over the primitives
// it stands for, built as the scene bound is and padded with the scene bound's own pad, fp32, rounded
// outward.  ids: the primitive IDs of a unit's slots.  on = false (n and ids still filled where the
// order has them): the scene has planes, vertex-normal triangles, more than kMaxUnits units, an order
// past GroupRec's counts, or no finite bound.
struct FlatUnits {
    bool on = false;
    int n = 0;
    std::vector<std::vector<int>> ids;
    std::vector<float> lo, hi; // 3 per unit
};
FlatUnits make_flat_units(const std::vector<HostPrim>& H, const BruteOrder& flat, const SceneBound& bound, int n_planes,
                          int n_vn);
// Which axis-aligned rectangles become outer records (out: per primitive, or empty for none).
void select_outer(const std::vector<HostPrim>& H, std::vector<char>& out);

} // namespace rtc
