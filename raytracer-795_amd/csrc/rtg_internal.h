// rtg_internal.h — layouts shared by the host scene builder (rtg_host.cpp) and the
// HIP kernels (rtg_device.hip).  Everything here is device-resident, read-only data
// laid out for gfx950 gathers, plus the per-level wavefront queue records.
#pragma once
#include <climits>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/rtg.h"

namespace rtg {

constexpr int kMaxLights = 64;      // per-node shadow slots are statically strided
constexpr int kStackDepth = 32;     // reference BVH depth cap 30 (src/BVH.cpp:55,67) + root
// The first 16 traversal-stack entries of a lane live in LDS (4 KB per 64-lane block), deeper ones
// (up to kStackDepth: the reference-tree fallback can need 31) in the lane's scratch: with the
// traversal kernels at 6 waves per SIMD, dragon 33.0 -> 31.6 ms, cornell_pt 392.8 -> 364.3 ms per
// frame (round 3, profiles/history/r3_ab_ldsstack.jsonl; 32 entries in LDS held them at 5 waves).
constexpr int kLdsStack = 16;       // traversal-stack entries per lane in LDS; deeper ones in scratch
constexpr int kTraceBlock = 64;     // threads per traversal block (LDS stack: 128 B per lane)
constexpr int kShadeBlock = 512;    // k_shade (simple variants): one queue atomic per block
constexpr int kTlasMinEntries = 16; // top-level BVH over objects / instances from this many entries on
constexpr int kTlasMaxDepth = 14;   // TLAS leaves at this depth take every remaining entry ...
constexpr int kTlasStack = 16;      // ... so a near-first walk never pushes more than this
constexpr int kTlasNoPrune = 0x40000000;   // TLAS child ref flag: no distance / behind-origin pruning

// One top-level entry of BVHMethods::FindIntersection's loop (src/Helper.cpp:32-73):
// objects first, then instances.  Read with scalar loads (wave-uniform loop).
struct TopObject {
    float inv[16];          // glm::inverse(model), column-major
    float invT[16];         // glm::inverseTranspose(model)
    float blur[3];
    int kind;               // 0 = sphere, 1 = triangle BVH (Triangle or Mesh)
    int material;           // 1-based (instance override applied)
    int geom;               // index of the geometry (base mesh for instances)
    int is_instance;
    int ident;              // 1: inv is exactly the identity (+0 off-diagonal) and blur is +0; 2: a sphere's
                            // inv is the identity up to zero signs and its blur zero (rtg_host.cpp;
                            // traversal only, transform_ray's strict)
    int wbox;               // wlo / whi valid: a transformed entry's world box (root box + eps overhang
    float wlo[3], whi[3];   // through the model matrix, blur sweep for times in [0, 1], margins)
    int grouped;            // a member of the flat group (SceneView::gents): fast rays test it there
    // round 6: a transformed mesh entry (wbox) whose world-space bounding sphere is much tighter than its
    // world box: centre + squared radius (vertices through the model matrix, blur sweep, the eps
    // overhang and margins); the object loop skips the entry for a lane whose ray line misses it
    int bsph;
    float bs[4];
};
// A sphere entry's test data (SceneView::tsph, one per entry, round 6): the object loop tests a sphere
// from this 32-byte record, whose address depends only on the entry index -- not on a dependent load
// of its Geometry record through TopObject::geom.  c = centre, radius; prim = its primitive, -1 none.
struct SphereEnt {
    float4 c;
    int prim, pad_[3];
};

// The flat group (round 5, closest_hit): the identity-transform entries whose mesh is tested without a
// node -- a root leaf, a reference root over two leaves, or a one-node traversal tree (<= kFlatMaxPrims
// triangles each) -- with their triangles in one array in the traversal-record format (p2.y reference
// position, p2.z first position of its reference leaf, p2.w gate flag).  Fast rays filter all of them
// at once and run the exact test on their own candidates only.
constexpr int kGroupMaxTris = 32;   // candidate bits of a lane
constexpr int kGroupMaxEnts = 16;
struct GroupEnt {
    int entry;              // top-level index
    int first, count;       // range in SceneView::gtris (= bits of the candidate mask)
    int root_box;           // 1: the reference root is interior (its box decides reachability)
    float root_min[3], root_max[3];
    int win;                // win_min / win_max valid (Geometry::win): a lane whose parameter window misses
    float win_min[3], win_max[3];   // this box has no candidate here, and a wave with no such lane skips the entry
};

// Per geometry (one per object; instances share their base mesh's geometry).
struct Geometry {
    int type;               // rtg_object_type
    int node_base;          // absolute index of the BVH root in the node array (-1 if root is a leaf)
    int sah_base;           // root of the traversal tree (SceneView::snodes), -1: reference-tree walk
    int root_leaf_start;    // absolute prim range when the root is a leaf (no box test)
    int root_leaf_count;    // -1: no primitives at all
    float root_min[3];      // root box (tested only when the root is interior)
    float root_max[3];
    int prim_base;          // absolute index of BVH position 0
    int nprims;
    float prune_pad;        // max distance a hit point can lie outside its primitive's box
    float win_min[3];       // root box widened by prune_pad, rounded outwards: every candidate
    float win_max[3];       // lies inside (window pruning of the whole object, visit_object)
    int num_textures;
    int textures[2];        // 1-based
    int texture_offset;
    int smooth;
    // sphere
    float center[3];
    float radius;
    int center_index;       // 1-based vertex index
    int win;                // window-test the root box before the walk (meshes of >= RTG_WIN_MIN_PRIMS)
    int flat_first;         // flat_count > 0: test the mesh's <= kFlatMaxPrims triangles without a node
    int flat_count;         // (visit_object): flat_split < 0 -- a one-node traversal tree, stris[flat_first ..];
    int flat_split;         // >= 0 -- a reference root over two leaves, tris[flat_first .. flat_split) and
                            // [flat_split .. flat_first + flat_count) (absolute positions)
};

// 64-byte BVH2 node holding both children's boxes (the reference tests a node's own box
// when it is visited; testing the child's box from its parent is the same predicate).
// a = {Lmin.xyz, Lmax.x}, b = {Lmax.yz, Rmin.xy}, c = {Rmin.z, Rmax.xyz},
// d = {lref, rref, lcount, rcount}: count 0 -> interior child (ref = absolute node index),
// count > 0 -> leaf child with prims [ref, ref+count) (absolute), count < 0 -> null child.
// A leaf child's box is the range box of its primitives, used only for pruning.
struct Node {
    float4 a, b, c;
    int4 d;
};

// 128-byte 4-wide node of a traversal tree (SAH over the triangle boxes, rtg_host.cpp
// sah_collapse).  Per-slot boxes in SoA form.  info: < 0 empty; 0 interior (ref = absolute Node4
// index); > 0 leaf of `info` triangles starting at ref (absolute index into SceneView::stris).
struct Node4 {
    float4 lox, loy, loz, hix, hiy, hiz;
    int4 ref;
    int4 info;
};

// Triangle in BVH order: the Cramer-rule operands of Triangle::bvhIntersect
// (src/Shape.cpp:299-316): a, a-b, a-c.  w lanes: x = original face index.
struct TriGeom {
    float4 p0;  // a.xyz, (a-b).x
    float4 p1;  // (a-b).yz, (a-c).xy
    float4 p2;  // (a-c).z, then (c-b).xyz in the reference-order copy (flat shading normal,
                // hit_record); the traversal copy (stris) holds the reference position, the first
                // position of its reference leaf and the gate flag (int bits) there
};

// Internal light types of hw7 object lights (appended after the scene's lights; only the
// path tracer's NEE loop reaches them).  inten = radiance; mesh: coverage = total world area,
// tri_first/tri_count = range in SceneView::emit_tris / emit_cdf; sphere: pos = world centre,
// size = world radius.
constexpr int kLightEmitMesh = 16;
constexpr int kLightEmitSphere = 17;
struct LightDev {
    int type;
    float pos[3], dir[3], inten[3];
    float coverage, fall, size;
    float normal[3], u[3], v[3];
    int tex;
    float cos_fall, cos_cov;   // host-computed cos() of fall/coverage (same convention)
    int tri_first, tri_count;  // mesh emitters
};

struct TextureDev {
    int kind, decal, interp, nc, normalizer;
    float noise_scale, bump;
    int w, h;
    long long texel_offset;    // into the texel pool (floats)
};

struct MaterialDev {
    int type, brdf, phong_exp, is_rough;
    float roughness;
    float ambient[3], diffuse[3], specular[3], mirror[3];
    float refraction_index, absorption_index;
    float absorption[3];
};

// Everything a kernel needs, passed by value.
struct SceneView {
    const TopObject* tops; int num_tops; int num_objects;
    const Geometry* geoms;
    const Node* nodes;
    const Node4* snodes;           // traversal trees (SAH, 4-wide)
    const TriGeom* stris;          // their triangles in leaf order; p2.y = reference position (int bits),
                                   // p2.z = first position of its reference leaf, p2.w = 1 if gated
    const float* gates;            // per reference position: min xyz, max xyz of its leaf's parent box
    const TriGeom* tris;
    const int4* prim_idx;          // BVH order: {v1,v2,v3 (1-based), smooth}; spheres {c,0,0,0}
    const float* vertices;         // xyz
    const float* vnormals;         // xyz
    const float* texcoords;        // uv
    int num_texcoords;
    const MaterialDev* materials; int num_materials; int child_split;   // child_split: queue_slots (below; in former padding)
    const TextureDev* textures; int num_textures; int absorb_skip;   // absorb_skip: term_absorbed (below; in former padding)
    const float* texels;
    const LightDev* lights; int num_lights;
    int max_depth;
    float shadow_eps, int_eps;
    float background[3], ambient[3];
    int bg_texture, env_light;
    int full;                      // 0: no textures / BRDFs / area or environment lights
    int spot;                      // any spot light (its double-precision cone math is compiled in)
    int heavy;                     // a spot or environment light: the full shading variants compile in
                                   // their double-precision libm code only then (light_sample)
    int brdf_only;                 // full only because of BRDFs (no textures / area / environment)
    int brdf_ts;                   // a Torrance-Sparrow (TS / TSF) material: the path tracer's BRDF variants
                                   // compile those models in only then
    int tex;                       // any textured object or BRDF material (k_shade's TEX variant)
    int meta_free;                 // Whitted: no RNG below level 0 (no textures / area / environment
                                   // lights / rough materials): child rays need no RayMeta (their
                                   // depth is max_depth - level, slot and path are unused)
    int lean_shadow;               // one point / spot / directional light: a Whitted shadow query
                                   // stores only origin + contribution (k_shadow rebuilds d, tmax, L)
    int lit_nodes;                 // one light, < kNodeMatMax materials: Whitted nodes store their lit
                                   // colour and k_shadow restores the ambient term if blocked
    int pnt_all;                   // k_shade stores every hit point: a dielectric material absorbs
                                   // (Beer's law reads refracted children's points) or eps >= 1e17
    int has_blur;                  // some object / instance has a nonzero motion-blur vector: the
                                   // ray queues carry times (RayQ::t)
    int bary;                      // some triangle is smooth-shaded or textured: the render path's
                                   // hit records carry the winner's barycentrics (HitPlanes::bg)
    int uni_walk;                  // camera-sample waves may walk the traversal tree wave-uniformly
                                   // (rtg_build_opts.uniform_walk; off: per-lane walks, for the parity
                                   // test that the two agree)
    // hw7 path tracer (per render: the host sets pt_flags and, with NEE, counts the object
    // lights into num_lights)
    const int* top_emit;           // per top-level entry: emitter light index, -1 if not a light
    const float* emit_tris;        // 9 floats per world-space emitter triangle (parse order)
    const float* emit_cdf;         // running float sum of the triangle areas per emitter
    int num_emit;
    int pt_flags;
    // top-level BVH over the entries (Node layout: count 0 = interior child, > 0 = leaf holding
    // entries tlas_idx[ref .. ref+count)); tlas_root -1: the reference's linear loop
    const Node* tlas;
    const int* tlas_idx;
    int tlas_root;
    float tlas_k[3];               // gett() error scale of the axis-aligned entries (closest_hit)
    // the flat group (GroupEnt); num_gents 0: none (top-level BVH scenes never group)
    const TriGeom* gtris;
    const GroupEnt* gents;
    const SphereEnt* tsph;         // per top-level entry: sphere test data (SphereEnt)
    const TopObject* gtop;         // a copy of the first member's entry: the members' common transform, one
                                   // load away (not gents[0].entry -> tops[], round 6)
    int num_gtris, num_gents;
};

// Path state of one path-tracing ray (per level, next to the RayQ planes / RayMeta).
struct PathRec {       // 16 B
    float tr, tg, tb;  // throughput (after the Beer attenuation of the segment, once shaded)
    int flags;         // bit 0: previous bounce specular; bits 8..: medium material (1-based, 0 none)
};

// One batch ("pass") of the frame: pixels [p0, p0 + npass) of the tiled pixel order (8x8, or 16x4 / 32x2 / 64x1 for row-block shards;
// blocks over the rank's owned rows) x samples [s0, s0 + ns).  Ray slot = (t - p0) * ns + (s - s0):
// all samples of a pixel are adjacent, so a wavefront traces near-identical rays.
struct PassDev {
    int s0, ns, p0, npass;
    int row_offset, row_stride, rows_owned, row_block;
    int tile_h;        // pixel tile height: 8, or the shard's row block when that is smaller
    int tile_s;        // tiles per column of a band (the band is tile_s * tile_h rows high)
};

// n / d for n >= 0, d > 0: a shift when d is a power of two (round 6: the pixel order's and the shards'
// divisors -- tile widths, 64-pixel tiles, full-band columns, samples per pixel, row blocks of 1 or 4,
// one shard -- are powers of two except at the image's last band / column; a 32-bit division is ~30
// VALU instructions, and the slot -> pixel map runs for every ray of every shading kernel)
__host__ __device__ inline int idiv(int n, int d) {
    return (d & (d - 1)) == 0 ? (n >> __builtin_ctz((unsigned)d)) : n / d;
}
// Shard row ownership (rtg_render_opts.row_block): owned row k <-> image row y.
__host__ __device__ inline int shard_row(int k, int off, int stride, int block) {
    const int b = idiv(k, block);
    return (b * stride + off) * block + (k - b * block);
}
// owned index of image row y, or -1 when another shard owns it
__host__ __device__ inline int shard_owned_index(int y, int off, int stride, int block) {
    const int b = idiv(y, block);
    const int q = idiv(b, stride);
    if (b - q * stride != off) return -1;
    return q * block + (y - b * block);
}

struct CameraDev {
    float pos[3], gaze[3], up[3], right[3];
    float l, r, b, t, dist;
    int nx, ny;
    float nxDA, nyDA, pw, ph, sw, sh;
    int sample_count, total;
    int dof;
    float focus, aperture;
};

// Wavefront queue records -------------------------------------------------------
// Queued rays (the Ray of src/Ray.h) as planes: a = (o.xyz, d.x), b = (d.y, d.z), t = time.  24 B
// per ray, 28 with times: the time plane is left out (t = nullptr, every time reads 0) when no
// object or instance has a motion-blur vector -- then the time cannot change any result, since
// transform_ray multiplies it by a zero blur and render-path times are finite.  Every queued ray
// is a closest-hit query without a distance bound (tmax = FLT_MAX).
struct RayQ {
    float4* a;
    float2* b;
    float* t;
};
constexpr size_t kRayBytes = 28;    // allocation per queued ray (the three planes)
inline RayQ ray_planes(void* base, long long cap, bool times) {
    char* p = static_cast<char*>(base);
    return RayQ{reinterpret_cast<float4*>(p), reinterpret_cast<float2*>(p + 16 * cap),
                times ? reinterpret_cast<float*>(p + 24 * cap) : nullptr};
}
struct RayMeta {        // 16 B
    int slot;           // sample slot in the batch
    unsigned path_lo, path_hi;
    int depth;          // remaining recursion depth (RecursiveShading's `depth`)
};
struct HitRec {         // 16 B
    int obj;            // top-level index, -1 miss
    int prim;           // BVH-order absolute prim index
    float t;            // gett distance
    int pad;
};
// The render path's hit records (k_trace -> k_shade / k_pt_shade): (object, primitive) per ray, 8 bytes.
// k_shade re-runs the winning test (hit_record); storing the test's ray parameter and barycentrics
// instead was measured slower (round 3, DESIGN.md §4 "hit records").
struct HitPlanes {
    int2* id;       // obj, prim
};
constexpr size_t kHitBytes = 8;
__host__ __device__ inline HitPlanes hit_planes(void* base, long long) {
    return HitPlanes{reinterpret_cast<int2*>(base)};
}

enum NodeKind : int {
    NK_FINAL = 0,       // color final (basic-only leaf, background, replace_all, miss)
    NK_MIRROR = 1,
    NK_DIEL_ENTER = 2,
    NK_DIEL_TIR = 3,
    NK_DIEL_EXIT = 4,
    NK_CONDUCTOR = 5
};

struct NodeRec {        // 48 B, one per traced ray
    float px, py, pz;   // world hit point ((0,0,0) on a miss, src/Helper.cpp:21)
    float cr, cg, cb;   // basic shading, then the resolved color
    int kind;
    float F;            // dielectric Fresnel / conductor Fresnel
    int child0, child1; // refracted / reflected child index in the next level (-1 none)
    int material;
    int slot;
};

// Whitted path: a level's n node records as three planes in the same 48 n bytes (structure of
// arrays), so the kernels that only need a node's colour (accumulate, light sums, final nodes in
// resolve) read 16 B of it, and k_shade stores the point only for hits and the links only for
// non-final nodes.  The path tracer uses the same planes for nodes with traced shadow queries only:
// colour + kind, point + index of the last traced light, throughput + radiance target (PtRad).
struct NodePlanes {
    float4* col;    // cr, cg, cb, kind (int bits; kNodeHit set for hits)
    float4* pnt;    // px, py, pz, F               (hit nodes only)
    int4* link;     // child0, child1, material, -  (kind != NK_FINAL only)
};
constexpr int kNodeHit = 0x400;
constexpr int kNodeFar = 0x800;    // hit point with a coordinate >= 1e18 or not finite (k_resolve)
// Single-light Whitted path (round 5, SceneView::lit_nodes): a node whose shadow query is traced
// stores its lit colour (ambient + the light's term) and its material index in the kind word's bits
// 12..30; k_shadow rewrites the colour to the ambient term only for a blocked query.  Scenes with more
// materials keep the contribution plane (lit_nodes = lean_shadow = 0).
constexpr int kNodeMatShift = 12;
constexpr int kNodeMatMax = 1 << 19;
inline NodePlanes node_planes(NodeRec* base, long long n) {
    float4* b = reinterpret_cast<float4*>(base);
    return NodePlanes{b, b + n, reinterpret_cast<int4*>(b + 2 * n)};
}

struct ShadowRec {      // 48 B per query (the allocation unit of a level's shadow planes)
    float4 o;           // origin.xyz, time
    float4 d;           // direction.xyz, dl = |p - light point| (modes 1 / 3; k_shadow rebuilds the t bound)
    float4 c;           // contribution rgb, mode (0 none, 1 distance test, 2 any hit, 3 object light)
};

// A level's shadow records as planes (round 6): the origin per shading node (o[i]; the lean
// single-light path stores it as 12-byte records), direction + light distance and contribution per
// query, LIGHT-MAJOR: query (node i, light li) at li * nn + i, so the queries of one light that a
// wave traces (the list is light-major within a wave) read consecutive records -- node-major
// (i * nLights + li) left every 128-byte line of d / c half used by a wave (C5: 142 B per query).
// No light-point plane: k_shadow's blocking tests need only dl, and the query's mode follows from
// the light's type (shadow_mode).
struct ShadowPlanes {
    float4* o;      // origin.xyz, time                      (per node)
    float4* d;      // direction.xyz, dl                     (per query)
    float4* c;      // contribution rgb, mode                (per query; several lights: k_shadow zeroes the
                    // mode of a blocked query)
    int nn;         // nodes of the level: the light stride of d / c
};
inline ShadowPlanes shadow_planes(ShadowRec* base, int nodes, int lights) {
    float4* b = reinterpret_cast<float4*>(base);
    const long long cap = (long long)nodes * (lights > 1 ? lights : 1);
    return ShadowPlanes{b, b + nodes, b + nodes + cap, nodes};
}

struct Counters {
    unsigned long long node_visits, tri_tests;           // closest-hit kernel
    unsigned long long shadow_node_visits, shadow_tri_tests;
    unsigned long long trace_lane_slots, shadow_lane_slots, trace_steps, shadow_steps;
    // shadow queries found blocked, and the node steps / triangle tests they took (the rest of
    // shadow_steps / shadow_tri_tests went to unblocked queries)
    unsigned long long shadow_blocked, shadow_blocked_steps, shadow_blocked_tris;
    // top-level entries visited by the lanes, and 64 x the entries each wave's loop went through
    unsigned long long trace_entry_visits, trace_entry_slots, shadow_entry_visits, shadow_entry_slots;
    // blocked shadow queries: histograms (bins 0, 1, 2, 3-4, 5-8, 9-16, 17-32, >32) of the node steps
    // taken before the blocker was accepted and after it, and the summed steps before
    unsigned long long shadow_hist_before[8], shadow_hist_after[8], shadow_blocked_steps_before;
    unsigned long long shadow_blocked_steps_before_wavemin;
    // wave cycles (s_memtime) spent per top-level entry of the linear object loop (entries >= 15 pooled
    // in the last slot), closest-hit and shadow kernels: where the traversal's time goes
    unsigned long long trace_entry_cycles[16], shadow_entry_cycles[16];
    // k_pt_shade wave cycles by phase: hit set-up, next-event estimation, continuation, compaction + stores
    unsigned long long pt_shade_cycles[4];
    // the flat group (round 6): lane work (triangle tests the lanes ran) and slots (64 x the tests their
    // waves ran), and its wave cycles split into set-up and tests
    unsigned long long trace_group_work, trace_group_slots, shadow_group_work, shadow_group_slots;
    unsigned long long trace_group_cycles[2], shadow_group_cycles[2];
};

// The path tracer's radiance (round 6): the running sum L of a sample travels with its
// path.  k_pt_shade reads it from the ray's queue slot (carry_in[i]; a new sample starts from (0,0,0)).
// A vertex whose contribution is final there (no traced shadow query) adds T (x) v itself and hands L
// to its continuation (carry_out at the child's queue index) or, the path's last vertex, writes
// rad[slot]; a vertex with traced queries leaves L in its own queue slot (carry_in[i], read by then)
// and its last light's query in k_shadow (per-light launches, in light order) writes L + T (x) v to the
// target -- node-indexed, so k_shadow loads it with the node's other records in one round, and the
// last light's launch (every query in it is its node's last) loads all of them unconditionally.  No
// per-level gather kernel.  lcnt: the level's per-light shadow-list counts (light li's list at
// slist + li * n).
struct PtRad {
    float4* carry_in;
    float4* carry_out;
    float4* rad;
    unsigned* lcnt;
    int light;          // k_shadow: the light of this launch's list (its entries are light * n + node)
};
constexpr size_t kCarryBytes = 16;    // float4 per queued ray

// The bounding-sphere radius of a transformed mesh entry (TopObject::bs[3]; entry_bounding_sphere, rtg_host.cpp):
// the largest squared distance from the centre c0 of any triangle corner taken through the model matrix, in
// double.  One function for the host pass (scene builds) and the kernel (rtg_radius.hip, rtg_scene_update), so
// both evaluate the same expressions in the same order: corner 0 is p0.xyz, corners 1 and 2 are p0 - e1 and
// p0 - e2; per corner the three row sums M v + M[3] - c0, left to right, and their squares added in order.
// Host and device are built with -ffp-contract=off, double add and multiply are IEEE on both, and the
// "NaN wins" maximum does not depend on the order of its operands (every value is a sum of squares: no -0;
// any NaN result means "no sphere"), so the two sides agree bit for bit.
struct RadiusXf {
    double m[4][3];     // the model matrix's columns (glm m[col][row], rows 0-2), widened from float
    double c0[3];
};
__host__ __device__ inline double radius2_fold(double mx2, double v) { return v > mx2 || v != v ? v : mx2; }
__host__ __device__ inline double tri_radius2(const TriGeom& tg, const RadiusXf& X, double mx2) {
    const double a[3] = {tg.p0.x, tg.p0.y, tg.p0.z};
    const double e[2][3] = {{tg.p0.w, tg.p1.x, tg.p1.y}, {tg.p1.z, tg.p1.w, tg.p2.x}};
    for (int q = 0; q < 3; q++) {
        double v[3], d2 = 0.0;
        for (int z = 0; z < 3; z++) v[z] = q == 0 ? a[z] : a[z] - e[q - 1][z];
        for (int r = 0; r < 3; r++) {
            const double w = X.m[0][r] * v[0] + X.m[1][r] * v[1] + X.m[2][r] * v[2] + X.m[3][r] - X.c0[r];
            d2 += w * w;
        }
        mx2 = radius2_fold(mx2, d2);    // NaN propagates (no sphere)
    }
    return mx2;
}
// The kernel's launcher: tris = n records on the device (n >= 1), part = kRadiusPartials doubles of device
// workspace; *r2 = the maximum (synchronous).  ms (may be null): the two launches' device time from HIP events.
constexpr int kRadiusBlock = 256;
constexpr int kRadiusMaxBlocks = 1024;
constexpr int kRadiusPartials = kRadiusMaxBlocks + 1;
int entry_radius2_device(const TriGeom* tris, int n, const RadiusXf& X, double* part, double* r2, float* ms,
                         std::string& err);

// What a built scene keeps for rtg_scene_update: the inputs of the top-level phases that do not
// depend on the free part of the descriptor, and the update's own state.  The build fills the kept inputs in its
// SceneArrays (rtg_host.cpp) and hands them over at its end; an update takes them back for the phases.
//
// The reference-order records of the meshes that may join the flat group (<= kFlatMaxPrims triangles), with each
// position's leaf (tie order) and gate flag: object i's nprims rows start at first[i] (-1: none kept).
struct SmallMeshes {
    std::vector<int> first;
    std::vector<TriGeom> tris;
    std::vector<int> pos_leaf;     // the first position of the record's reference leaf (scene-wide) ...
    std::vector<char> pos_gated;   // ... and whether that leaf's parent (gates[]) is not the root
};
// An is_light object's object-space corners in parse order, xyz each (object_lights): a sphere's centre, else
// three per triangle.
struct EmitSource {
    int object;
    std::vector<float> corners;
};
// The frozen part of the descriptor a scene was built from: rtg_scene_update refuses a descriptor that differs
// in it.  Pointers are not kept (texels is null in `textures`).
struct FrozenDesc {
    int num_vertices = 0, num_texcoords = 0, num_faces = 0, num_materials = 0;
    float intersection_test_eps = 0.0f;
    std::vector<rtg_object_desc> objects;
    std::vector<rtg_instance_desc> instances;
    std::vector<rtg_texture_desc> textures;
};
struct SceneUpdate {
    std::vector<Geometry> geoms;
    std::vector<char> geom_finite;   // per object: every primitive box coordinate finite
    SmallMeshes small;
    std::vector<EmitSource> emit;
    std::vector<TriGeom> all_tris;   // a host-only scene: every reference-order record (a device scene's are in d_tris)
    FrozenDesc frozen;
    double* d_radius = nullptr;      // device: the radius kernel's partials (kRadiusPartials), from the first update on
    uint64_t top_hash = 0;           // rtg_scene_top_hash: of the last build or update
    bool broken = false;             // an update failed after its device work began: destroy only
};


// Host-side launchers (rtg_device.hip) ------------------------------------------------
// Where a render's samples go.  rtg_render*: the scene's accumulator, the camera's whole sample range,
// nothing accumulated before, no moments (target == nullptr).  A frame (rtg_frame_add_samples): its own
// accumulator, samples [s0, s0 + ns) of the camera's, behind `have` samples the accumulator already holds.
struct RenderTarget {
    float* acc;       // running float32 sums, 3 per owned pixel in owned-row order
    float* mom;       // mean and M2 of the samples' luminance, 2 per owned pixel, or null
    int s0, ns;       // the window of the camera's samples this call traces
    int have;         // samples already in acc / mom
    // Adaptive frames.  active: the frame's active pixels as ascending tile-order
    // indices (device; null = every owned pixel), nactive of them: the render loop then runs over
    // pixel ordinals [0, nactive) and the kernels look the pixel up (PassDevA::active).  s0 / ns / have
    // count positions of the sample order: position j traces sample (j * ord_m) % ord_n (ord_m 0: j).
    const int* active = nullptr;
    int nactive = 0;
    int ord_m = 0, ord_n = 1;
};
// A pass of an adaptive frame: PassDev plus the active list (pixel ordinal p0 + i is the pixel at tile-order
// index active[p0 + i]; null: the ordinal itself) and the sample order.  The kernels that turn a slot into
// a pixel and a sample are templates over the pass type, so the instantiations rtg_render and plain frames
// launch (PassDev) carry neither the fields nor the branches: the launchers fall back to them whenever a
// PassDevA has no list and the identity order.
struct PassDevA : PassDev {
    const int* active = nullptr;
    int ord_m = 0, ord_n = 1;
    bool plain() const { return !active && !ord_m; }
};
// A pass over caller-supplied primary rays (rtg_render_rays): PassDev plus the caller's array,
// read in place.  Slot -> pixel and sample as a PassDev; the primary ray of (pixel, sample) is
// rays[pixel * nsamp + sample] (64-bit index) instead of the camera's.  A third pass type, so that no PassDev /
// PassDevA instantiation carries the pointer or a branch on it; only the kernels that generate level 0 (GEN)
// are instantiated for it -- everything else about such a pass is a PassDev's and takes those kernels.
struct PassDevR : PassDev {
    const struct ::rtg_ray* rays;
    int nsamp;
};
template <class PS> inline constexpr bool kRayPass = false;
template <> inline constexpr bool kRayPass<PassDevR> = true;
// What the host hands the launchers: a PassDevA, or -- rays set -- a ray pass.  Host-side only: with_pass
// (rtg_device.hip) turns it into the type whose kernels the pass takes.
struct PassArg : PassDevA {
    const struct ::rtg_ray* rays = nullptr;
    int nsamp = 0;
};

// What one trace -> shade -> shadow step reads and writes: a level of a pass, or a step of the stream
// schedule (Render::step, rtg_host.cpp).  Each schedule fills it from its own buffers.
struct StepIO {
    RayQ rays;                    // queued rays [0, nq) (a pass's level 0: none)
    const RayMeta* meta;
    HitRec* hits;
    PathRec* paths;               // path tracer
    NodeRec* nodes;
    ShadowRec* shadows;
    int* slist;
    RayQ next_rays;               // the children the step queues, their count in the low word of *qcount (the
    RayMeta* next_meta;           // high word: the Whitted shadow list's entries)
    PathRec* next_paths;
    unsigned long long* qcount;
    int n;                        // rays of the step
    int nq, gbase;                // gen: rays [0, nq) are queued, ray i >= nq is the primary ray of slot gbase + i - nq
    bool gen;                     // the step holds primary rays, generated in the kernels (no level-0 ray buffer)
    int level;                    // a pass's level; 0 on the stream schedule, whose rays carry theirs:
    const unsigned char* lv_in;   // per-ray levels of a stream step (or null)
    unsigned char* lv_out;
    PtRad pr;                     // path tracer
    int uni_from;                 // shadow queries: first camera-sample node (wave-uniform walk), INT_MAX none
};
void launch_trace(const SceneView& sv, const CameraDev& cam, const PassArg& ps, uint64_t seed, const StepIO& io,
                  int exhaustive, Counters* ctr, hipStream_t st);
// queued rays only, full hit records (rtg_trace_closest): no camera, no pass
void launch_trace_queued(const SceneView& sv, const RayQ rays, HitRec* hits, int n, int exhaustive, hipStream_t st);
// ray queries on device arrays: n AoS rtg_ray records -> RayQ planes with times; out[i] = 1 iff
// ray i's closest hit has t < tmax[i] (tmax null: +inf), one byte per ray
void launch_pack_rays(const struct ::rtg_ray* rays, const RayQ q, int n, hipStream_t st);
void launch_occluded(const SceneView& sv, const RayQ rays, const float* tmax, unsigned char* out, int n, int exhaustive,
                     hipStream_t st);
// workspace of a device-array query per ray: the ray planes (kRayBytes) and a HitRec
constexpr size_t kQueryBytes = kRayBytes + 16;
#ifdef __HIPCC__
// closest_hit's ANYHIT flag (occlusion queries, k_occluded): the caller asks only whether the closest hit lies
// below tmax.  `nearest` starts at tmax and only decreases, and the top-level acceptance is strict, so a lane
// that has accepted an entry (h.obj >= 0) knows the answer whatever the remaining entries hold: it is done and
// skips them, and a loop ends when its wave has no undone lane left.  With the flag off (every other kernel)
// both are the constant false: those walks compile to what they were.
template <bool ANYHIT> __device__ __forceinline__ bool lane_done(const HitRec& h) {
    if constexpr (ANYHIT) return h.obj >= 0;
    else return false;
}
template <bool ANYHIT> __device__ __forceinline__ bool wave_done(const HitRec& h) {
    if constexpr (ANYHIT) return __ballot(h.obj < 0) == 0ull;
    else return false;
}
#endif
void launch_shade(const SceneView& sv, const CameraDev& cam, const PassArg& ps, uint64_t seed, const StepIO& io,
                  hipStream_t st);
void launch_pt_shade(const SceneView& sv, const CameraDev& cam, const PassArg& ps, uint64_t seed, const StepIO& io,
                     Counters* ctr, hipStream_t st);
void launch_shadow(const SceneView& sv, const StepIO& io, int exhaustive, Counters* ctr, unsigned* nan_queries,
                   hipStream_t st);
// the path tracer's queries: one launch per light, in light order (PtRad)
void launch_pt_shadow(const SceneView& sv, const StepIO& io, int exhaustive, Counters* ctr, unsigned* nan_queries,
                      hipStream_t st);
// the bottom-up step and the accumulation on explicit node planes (stream schedule: a step's nodes
// [0, count) against the next step's; the primaries of a pixel range at an offset of a step's planes)
void launch_resolve_planes(const SceneView& sv, const NodePlanes& self, const NodePlanes& child, int count,
                           hipStream_t st);
// mom (a frame's moments, or null): mean and M2 of each pixel's sample luminance (2 floats per owned
// pixel, in `acc` order), continued over this launch's samples; mom_k0 = samples they already hold
void launch_accumulate_planes(const SceneView& sv, const NodePlanes& level0, const NodePlanes& level1, bool resolve,
                              float* acc, const PassArg& ps, int nx, int mode, hipStream_t st, float* mom = nullptr,
                              int mom_k0 = 0);
void launch_resolve(const SceneView& sv, NodeRec* nodes, const NodeRec* child_nodes, int n, int n_child,
                    hipStream_t st);
// levels p (nodes) and p + 1 (child_nodes, resolved inline, not stored) against the resolved level p + 2
void launch_resolve2(const SceneView& sv, NodeRec* nodes, const NodeRec* child_nodes, const NodeRec* grand_nodes, int n,
                     int n_child, int n_grand, hipStream_t st);
// mode: 0 = continue the running sum, 1 = start from (0,0,0), 2 = assign (single-sample camera)
// level0 / level1 hold NodePlanes over n0 / n1 nodes; whitted: resolve level 0 against level 1
// level2 (optional): level 1 is resolved inline against it (the bottom-up pass left level 1 unresolved)
void launch_accumulate(const SceneView& sv, const NodeRec* level0, const NodeRec* level1, bool resolve, float* acc,
                       const PassArg& ps, int nx, int mode, hipStream_t st, bool whitted, int n0, int n1,
                       const NodeRec* level2 = nullptr, int n2 = 0, float* mom = nullptr, int mom_k0 = 0);
// A frame's error figures (rtg_frame_error_stats): per-block double partials of the per-pixel mean and
// standard error (3 doubles per block of 256 pixels in `part`: sum of means, sum of sems, max sem),
// combined by one block into out[0..2] (sums, max) -- no atomics, so the figures repeat
constexpr int kErrBlock = 256;
void launch_frame_error(const float* mom, int npix, int n, double* part, double* out, hipStream_t st);
void launch_finalize(const float* acc, float* out, int nx, int ny, int row_offset, int row_stride, int row_block, int total,
                     hipStream_t st);
// Adaptive frames.  cnt: one word per owned pixel in `acc` order -- kRetiredBit set
// once the pixel is retired, the low bits then hold the samples it keeps; an active pixel's word is 0
// (it holds the frame's samples_done).
constexpr unsigned kRetiredBit = 0x80000000u;
constexpr int kScanBlock = 256;
// counts-aware forms of launch_finalize / launch_frame_error: each pixel by its own count (`done` for
// the active ones)
void launch_finalize_counts(const float* acc, const unsigned* cnt, float* out, int nx, int ny, int row_offset,
                            int row_stride, int row_block, int done, hipStream_t st);
void launch_frame_error_counts(const float* mom, const unsigned* cnt, int npix, int done, double* part, double* out,
                               hipStream_t st);
// retire the active pixels that pass (double)var / n <= thr^2, thr = max(abs_tol, rel_tol * mean), n = done
void launch_frame_retire(const float* mom, unsigned* cnt, int npix, int done, float rel_tol, float abs_tol,
                         hipStream_t st);
// retire the active pixels whose byte of `mask` (device, owned-row order) is not 0
void launch_frame_retire_mask(const unsigned char* mask, unsigned* cnt, int npix, int done, hipStream_t st);
// The active list: the tile-order indices t in [0, npix) of the pixels not retired, ascending, and their
// number in part[nblk(npix, kScanBlock)] (part: one int per block of kScanBlock indices + 1).  Ballot
// prefixes, per-block counts, a scan of the counts, a scatter: no atomics, so the list repeats.
void launch_active_list(const unsigned* cnt, int npix, const PassDev& ps, int nx, int* part, int* active,
                        hipStream_t st);
void launch_hit_details(const SceneView& sv, const RayQ rays, const HitRec* hits, struct ::rtg_hit* out,
                        const int* orig_prim, int n, hipStream_t st);
// First-hit feature buffers (rtg_render_aov).  A pass's samples leave 32-byte records (rec_a:
// t, normal; rec_b: albedo, hit flag; one per slot, kAovRecBytes); k_aov_reduce sums a pixel's records in sample
// order into planes over the npix owned pixels in tile order (hits / depth [t]; normal / albedo / ids
// [c * npix + t]); k_aov_place turns them into the image layout ([e] and [3 * e + c] over the output's pixels,
// npix unused).
struct AovPlanes {
    int* hits;
    float* depth;
    float* normal;
    float* albedo;
    int* ids;
    size_t npix;
};
constexpr size_t kAovRecBytes = 32;
// ps: the pixel range [p0, p0 + npass) x the window [s0, s0 + ns), npass * ns < 2^31; rec_a / rec_b: npass * ns each
void launch_aov(const SceneView& sv, const CameraDev& cam, const PassDev& ps, uint64_t seed, int exhaustive,
                const int* orig_prim, float4* rec_a, float4* rec_b, const AovPlanes& out, hipStream_t st);
void launch_aov_place(const AovPlanes& in, const AovPlanes& out, int nx, int out_rows, const PassDev& ps, int compact,
                      hipStream_t st);
// rtg_camera_rays: ps is row-major (tile_h = tile_s = 1, no shard); out[i] = the ray of slot i, i < n
void launch_camera_rays(const CameraDev& cam, const PassDev& ps, uint64_t seed, int n, struct ::rtg_ray* out,
                        hipStream_t st);
// rtg_render_rays: *bad (device, preset to ~0) = the lowest index of `rays` whose ray is not
// finite or has a zero direction, over the rays of the shard's owned rows (nx * nsamp records per row)
void launch_check_rays(const struct ::rtg_ray* rays, int rows_owned, int nx, int nsamp, int row_offset, int row_stride,
                       int row_block, unsigned long long* bad, hipStream_t st);

// Traversal-tree build records (rtg_host.cpp sah_split, rtg_sah_gpu.hip): one triangle's box and face
// index (32 B; the centroid is the box centre), and the binned-SAH BVH2 node over a range of them.
constexpr int kSahBins = 16;
constexpr int kSahMaxLeaf = 4;
struct SahRec {
    float lo[3], hi[3];
    int idx, pad_;
};
struct SahNode2 {
    float lo[3], hi[3];
    int left, right;          // children (-1 for a leaf)
    int start, count;         // range in the SAH primitive order (interior nodes too)
};

// Multi-GPU rows gather: shard r's compact rows start at row prefix[r] of `recv`; every frame
// row y is copied from its owning shard ((y / block) % nranks).  nranks <= kMaxRanks.
constexpr int kMaxRanks = 64;
struct ShardPrefix { int rows[kMaxRanks + 1]; };
void launch_place_rows(const float* recv, float* frame, int nx, int ny, int nranks, int block, const ShardPrefix& pre,
                       hipStream_t st);

// Hooks between the C ABI's single-device driver (rtg_host.cpp) and the multi-GPU fan-out
// (rtg_multi.cpp).  rtg_scene is the opaque ABI handle (defined in rtg_host.cpp).
struct MultiState;
void multi_free(MultiState* m);
int set_error(int code, const std::string& msg);           // sets rtg_last_error() of this thread
int scene_device(const rtg_scene* s);
int scene_render(rtg_scene* s, const rtg_camera_desc* cam, const rtg_render_opts* o, float* out_dev, hipStream_t st);
rtg_render_stats scene_stats(const rtg_scene* s);
void scene_set_stats(rtg_scene* s, const rtg_render_stats& st);
MultiState*& scene_multi(rtg_scene* s);
int scene_replicate(rtg_scene* src, int device, rtg_scene** out);
int render_multi(rtg_scene* s, const rtg_camera_desc* cam, const rtg_render_opts* o, float* out_dev, hipStream_t st);

// Photographic tone mapping (rtg_tonemap.hip); hdr / out are device arrays.
int tonemap_white_index(int n, float burn_percent);
int tonemap_device(const float* hdr, int nx, int ny, const rtg_tonemap_desc& tm, float* out, hipStream_t st,
                   std::string& err);

// Edge-avoiding a-trous denoiser (rtg_denoise.hip); every pointer of `in` and `out` are device
// arrays, `o` holds the effective options (defaults resolved).
int denoise_device(const rtg_denoise_inputs& in, int nx, int ny, const rtg_denoise_opts& o, float* out, hipStream_t st,
                   std::string& err);
// The same over a workspace the caller keeps (denoise_workspace_bytes of device memory, 16-byte aligned);
// denoise_device allocates one per call and runs this.
size_t denoise_workspace_bytes(int nx, int ny);
int denoise_device_ws(const rtg_denoise_inputs& in, int nx, int ny, const rtg_denoise_opts& o, float* out, void* workspace,
                      hipStream_t st, std::string& err);
// rtg_frame_denoise's per-call inputs from a whole, uncompacted frame: rgb[3 * i + c] as
// launch_finalize / launch_finalize_counts resolve pixel i, variance[i] = (M2 / (float)(n - 1)) / (float)n for the
// pixel's own count n >= 2, else +0.  cnt NULL: every pixel holds `done`; variance NULL: none written, mom unread.
void launch_frame_inputs(const float* acc, const unsigned* cnt, const float* mom, int npix, int done, float* rgb,
                         float* variance, hipStream_t st);

// GPU BVH construction (rtg_bvh_gpu.hip): the reference median-split tree of one object.
// nodes: breadth-first {left, right, start, end} (children -1: none); box: 6 floats per node
// (min xyz, max xyz); perm: BVH position -> original primitive.  Inputs must be finite.
// Page-locked host array (hipHostMalloc): device-to-host copies into it run at DMA speed (the
// GPU build's 84 MB result for 1 M triangles: 16 ms into pageable vectors).
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        const hipError_t e = hipHostMalloc((void**)&p, sizeof(T) * count, hipHostMallocDefault);
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

// Page-locked staging from a process-wide pool: hipHostMalloc of the ~80 MB a 1 M-triangle build
// returns costs milliseconds per scene creation, so the buffers are kept and reused.
// get returns a buffer of at least `bytes` and its real capacity in *cap; put takes the capacity back.
void* pinned_pool_get(size_t bytes, size_t* cap);
void pinned_pool_put(void* p, size_t cap);
struct PooledPinned {
    void* p = nullptr;
    size_t cap = 0;           // the buffer's real capacity (>= the bytes last asked for)
    PooledPinned() = default;
    PooledPinned(const PooledPinned&) = delete;
    PooledPinned& operator=(const PooledPinned&) = delete;
    ~PooledPinned() { if (p) pinned_pool_put(p, cap); }
    bool get(size_t b) {
        if (p && cap >= b) return true;
        if (p) pinned_pool_put(p, cap);
        cap = 0;
        p = pinned_pool_get(b, &cap);
        return p != nullptr;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
// The GPU median-split build's result: nodes in breadth-first order (children after their parent) as
// 40-byte records {left, right, start, end, min xyz, max xyz} (the host's HNode layout), and the
// primitive permutation.
struct GpuBvh {
    PooledPinned perm;       // int[n]
    PooledPinned nodes;      // 40 B per node
    int num_nodes = 0;
    int root = -1;
};
int gpu_build_bvh(const float* centers, const float* bmin, const float* bmax, int n, GpuBvh& out, std::string& err,
                  hipStream_t st);
// GPU binned-SAH build of one mesh's traversal tree (rtg_sah_gpu.hip), collapsed to 4-wide nodes on the
// device as rtg_host.cpp collapse_node does (slot boxes widened by `pad`, leaf refs from tri_base, interior
// refs 0-based within the mesh, breadth-first): alloc4(count) returns host memory for the Node4 records
// (count 0: the root is a leaf); the face index of every SAH position into order_host[n]; the binary
// tree's node count and order-independent hash (sah_tree_stats).  Runs on its own non-blocking stream of
// the calling thread's current device.
int gpu_build_sah(const SahRec* recs_host, int n, int tri_base, float pad, const std::function<Node4*(size_t)>& alloc4,
                  int* order_host, uint64_t& bvh2_nodes, uint64_t& hash, std::string& err);
// Empty launches that load the GPU build's / the render kernels' code objects (scene-create warm-up).
void gpu_bvh_warm(hipStream_t st);
void device_warm(hipStream_t st);

// SceneView::child_split as rtg_scene_create sets it (rtg_host.cpp): on unless RTG_CHILD_SPLIT=0 is in the
// environment -- read per scene creation: a data switch for A/B runs and the tests, same device code.
int child_split_default();
// SceneView::absorb_skip likewise: on unless RTG_ABSORB_SKIP=0 is in the environment (term_absorbed, below).
int absorb_skip_default();

#ifdef __HIPCC__
// One light: the query's node is fl(amb + c) if the light is visible and amb if it is blocked (amb: the
// running sum, 0 + La*ka, never -0; c: the unshadowed term, c.w its mode).  Where fl(amb + c) has amb's bits in
// every channel the query need not be traced; integer compares, so a NaN term keeps its query.  Not applied
// with several lights.  `on`: SceneView::absorb_skip (RTG_ABSORB_SKIP=0 clears it).  DESIGN.md section 16.
__device__ __forceinline__ bool term_absorbed(int on, int num_lights, float ar, float ag, float ab, const float4& c) {
    if (!on || num_lights != 1 || !(c.w == 1.0f || c.w == 2.0f)) return false;
    return ((__float_as_uint(ar + c.x) ^ __float_as_uint(ar)) | (__float_as_uint(ag + c.y) ^ __float_as_uint(ag)) |
            (__float_as_uint(ab + c.z) ^ __float_as_uint(ab))) == 0u;
}

// k_shade's compaction of a level's child rays and shadow queries (shade_ray, rtg_device.hip; called by
// every thread of a BLOCK-thread block): ballot prefixes inside each wave, wave totals combined in LDS,
// one 64-bit atomic per block on the level's queue counter (low word: rays, high word: shadow entries).
// has0 / has1: the lane has a refracted / a reflected child; stot: the wave's shadow-list entries.
// Returns the lane's queue positions idx0 / idx1 and the wave's first shadow-list position sb.
// split (round 7): the block's range holds every wave's refracted children, then every wave's reflected
// ones; otherwise each lane's two children are adjacent, in wave and lane order, as before.
template <int BLOCK>
__device__ inline void queue_slots(bool split, bool has0, bool has1, unsigned stot, unsigned long long* qcount, int& idx0,
                                   int& idx1, unsigned& sb) {
    __shared__ unsigned s_wc[BLOCK / 64], s_ws[BLOCK / 64], s_w1[BLOCK / 64];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long lt = __lanemask_lt();
    const int nchild = (has0 ? 1 : 0) + (has1 ? 1 : 0);
    const unsigned long long m1 = __ballot(split ? has0 : nchild >= 1), m2 = __ballot(split ? has1 : nchild >= 2);
    const unsigned coff = __popcll(m1 & lt) + (split ? 0u : __popcll(m2 & lt));
    if (lane == 0) { s_wc[w] = __popcll(m1) + (split ? 0u : __popcll(m2)); s_w1[w] = __popcll(m2); s_ws[w] = stot; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0, sh = 0;
        for (int k = 0; k < BLOCK / 64; k++) {
            const unsigned a = s_wc[k], b = s_ws[k];
            s_wc[k] = c; s_ws[k] = sh;
            c += a; sh += b;
        }
        if (split)          // the reflected children's ranges, after every wave's refracted ones
            for (int k = 0; k < BLOCK / 64; k++) {
                const unsigned a = s_w1[k];
                s_w1[k] = c;
                c += a;
            }
        s_base = (c | sh) ? atomicAdd(qcount, ((unsigned long long)sh << 32) | c) : 0ull;
    }
    __syncthreads();
    idx0 = (int)((unsigned)s_base + s_wc[w] + coff);
    idx1 = split ? (int)((unsigned)s_base + s_w1[w] + __popcll(m2 & lt)) : idx0 + (has0 ? 1 : 0);
    sb = (unsigned)(s_base >> 32) + s_ws[w];
}

// Pixel ordinal -> tile-order index and position -> sample index of a pass (slot_pixel, accumulate_body):
// the identity for a PassDev; an adaptive frame's pass looks them up, wave-uniform branches.
__device__ __forceinline__ int pass_pixel(const PassDev&, int ordinal) { return ordinal; }
__device__ __forceinline__ int pass_sample(const PassDev&, int position) { return position; }
__device__ __forceinline__ int pass_pixel(const PassDevA& ps, int ordinal) { return ps.active ? ps.active[ordinal] : ordinal; }
__device__ __forceinline__ int pass_sample(const PassDevA& ps, int position) {
    return ps.ord_m ? (int)(((unsigned)position * (unsigned)ps.ord_m) % (unsigned)ps.ord_n) : position;
}

// Luminance of a colour as the tone mapper and a frame's moments (§14) define it:
// 0 when negative or not finite.
__device__ __forceinline__ float tm_lum(const float* c) {
    const float y = (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2];
    return (__builtin_isfinite(y) && y > 0.0f) ? y : 0.0f;
}
#endif

}  // namespace rtg
