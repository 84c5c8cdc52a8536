/*
 * rtg.h — C ABI of the MI355X-native render loop for the CENG795 XML ray tracer
 * (badiba/raytracer-795).  Plain C, plain pointers and sizes, no C++/torch types.
 *
 * Drop-in seam:
 *   reference  void Scene::renderScene(void)                       src/Scene.h:89, src/Scene.cpp:294-363
 *   reference  ReturnVal BVHMethods::FindIntersection(ray,objs,inst) src/Helper.h:25, src/Helper.cpp:18-80
 *
 *   rtg_scene_create()  replaces the precompute half of renderScene()
 *                        (Perlin table, ComputeObjectTransformations, smooth normals,
 *                        per-object BVH construction: src/Scene.cpp:296-323)
 *   rtg_render()        replaces the per-camera pixel loop of renderScene()
 *                        (8 std::threads of ThreadedRendering -> Single/MultiSample ->
 *                        Shading: src/Scene.cpp:329-362, 269-292, 365-411) and writes
 *                        the float RGB framebuffer the reference keeps in Image::_data
 *                        (src/Image.cpp:16-24) — [y][x][c], 0..255 scale, unclamped.
 *   rtg_trace_closest() replaces BVHMethods::FindIntersection for a batch of rays
 *                        (closest-hit with the reference's object/instance rules).
 *
 * The scene descriptor is exactly what the reference Parser leaves in the global
 * Scene after `new Scene(xml)` (src/Scene.cpp:455-504, src/Parser.h): raw vertices,
 * texture coordinates, objects with their transformation-reference lists, instances,
 * materials, textures (decoded texels), lights in the reference's light order, scalars.
 * All indices keep the reference's conventions: vertex / material / texture indices
 * are 1-based positions (materials[matIndex-1], src/Scene.cpp:375; vertices[idx-1],
 * src/Shape.cpp:300-302), transformation ids are 1-based positions into the per-kind lists
 * (src/Helper.cpp:158).
 *
 * Every function returns RTG_OK (0) or a negative rtg_status; rtg_last_error() returns
 * a thread-local message.  Nothing throws or aborts.  The library copies all inputs to
 * device memory at create time and keeps no pointer into caller memory after return.
 */
#ifndef RTG_H_
#define RTG_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTG_ABI_VERSION 10

typedef enum rtg_status {
    RTG_OK = 0,
    RTG_ERR_INVALID = -1,   /* malformed descriptor / argument */
    RTG_ERR_NO_DEVICE = -2, /* no usable gfx950 device */
    RTG_ERR_OOM = -3,       /* device or host allocation failed */
    RTG_ERR_HIP = -4,       /* HIP runtime error (message in rtg_last_error) */
    RTG_ERR_UNSUPPORTED = -5
} rtg_status;

/* ---- enums mirror src/defs.h:8-11, src/Material.h:7-8, src/Light.h:12, src/Transformation.h:7 ---- */
typedef enum rtg_object_type { RTG_OBJ_SPHERE = 0, RTG_OBJ_TRIANGLE = 1, RTG_OBJ_MESH = 2 } rtg_object_type;
typedef enum rtg_xform_type {
    RTG_XF_TRANSLATION = 1, RTG_XF_SCALING = 2, RTG_XF_ROTATION = 3, RTG_XF_COMPOSITE = 4
} rtg_xform_type;
typedef enum rtg_material_type {
    RTG_MAT_NORMAL = 0, RTG_MAT_MIRROR = 1, RTG_MAT_CONDUCTOR = 2, RTG_MAT_DIELECTRIC = 3
} rtg_material_type;
/* BRDFType order of src/Material.h:8 */
typedef enum rtg_brdf_type {
    RTG_BRDF_NONE = 0, RTG_BRDF_OBP = 1, RTG_BRDF_MBP = 2, RTG_BRDF_MBPN = 3, RTG_BRDF_OP = 4,
    RTG_BRDF_MP = 5, RTG_BRDF_MPN = 6, RTG_BRDF_TS = 7, RTG_BRDF_TSF = 8
} rtg_brdf_type;
/* DecalMode order of src/defs.h:8 */
typedef enum rtg_decal_mode {
    RTG_DECAL_REPLACE_KD = 0, RTG_DECAL_BLEND_KD = 1, RTG_DECAL_BUMP_NORMAL = 2,
    RTG_DECAL_REPLACE_NORMAL = 3, RTG_DECAL_REPLACE_ALL = 4, RTG_DECAL_REPLACE_BACKGROUND = 5,
    RTG_DECAL_NONE = 6
} rtg_decal_mode;
typedef enum rtg_interp { RTG_INTERP_NN = 0, RTG_INTERP_BILINEAR = 1 } rtg_interp;
typedef enum rtg_texture_kind { RTG_TEX_IMAGE = 0, RTG_TEX_PERLIN = 1 } rtg_texture_kind;
typedef enum rtg_noise_conv { RTG_NC_ABSVAL = 0, RTG_NC_LINEAR = 1, RTG_NC_NONE = 2 } rtg_noise_conv;
/* lights are given in the order the reference pushes them (src/Parser.h:1223-1314):
   all Point, then Directional, Spot, Area, SphericalDirectional (environment). */
typedef enum rtg_light_type {
    RTG_LIGHT_POINT = 0, RTG_LIGHT_AREA = 1, RTG_LIGHT_DIRECTIONAL = 2, RTG_LIGHT_SPOT = 3,
    RTG_LIGHT_ENVIRONMENT = 4
} rtg_light_type;

/* One entry of an object's <Transformations> list, e.g. "t1 s2 r1" (src/Parser.h:769-796).
   index is the 1-based position in the list of that kind. */
typedef struct rtg_xform_ref { int32_t type; int32_t index; } rtg_xform_ref;

typedef struct rtg_object_desc {
    int32_t type;            /* rtg_object_type */
    int32_t id;              /* XML id (MeshInstance baseMeshId lookup, src/Parser.h:1181-1186) */
    int32_t material;        /* 1-based material position */
    int32_t num_textures;    /* 0..2 (src/Parser.h:830-853) */
    int32_t textures[2];     /* 1-based texture positions */
    int32_t texture_offset;  /* Mesh: xml textureOffset - vertexOffset (src/Parser.h:1147); others 0 */
    int32_t smooth;          /* Mesh shadingMode="smooth" (src/Parser.h:958-974); ignored otherwise */
    int32_t xform_first;     /* range in rtg_scene_desc.xform_refs */
    int32_t xform_count;
    float blur[3];           /* MotionBlur translation (src/Parser.h:856-861), 0 if absent */
    /* sphere */
    int32_t center;          /* 1-based vertex index */
    float radius;
    /* triangle */
    int32_t v[3];            /* 1-based vertex indices */
    /* mesh */
    int32_t face_first;      /* range in rtg_scene_desc.faces (triples of 1-based vertex indices,
                                vertexOffset already added: src/Parser.h:1109-1149) */
    int32_t face_count;
    /* object light (hw7 <LightSphere> / <LightMesh>, pages/Page7.md:7-13; no reference code):
       is_light = 1 makes the object an emitter of `radiance` from both sides.  Only the path
       tracer (rtg_camera_desc.integrator) treats it as a light; the reference integrator
       shades it like any other object. */
    int32_t is_light;
    float radiance[3];
} rtg_object_desc;

typedef struct rtg_instance_desc {
    int32_t base_object;     /* 0-based index into objects (a Mesh) */
    int32_t id;
    int32_t material;        /* 1-based; overrides the base mesh material (src/Helper.cpp:68) */
    int32_t reset_transform; /* src/Helper.cpp:216-218 */
    int32_t xform_first;
    int32_t xform_count;
    float blur[3];
} rtg_instance_desc;

typedef struct rtg_material_desc {   /* src/Material.h:10-33, src/Parser.h:304-474 */
    int32_t type;            /* rtg_material_type */
    int32_t brdf;            /* rtg_brdf_type */
    int32_t phong_exp;
    int32_t is_rough;
    float roughness;
    float ambient[3];
    float diffuse[3];
    float specular[3];
    float mirror[3];
    float refraction_index;
    float absorption_index;
    float absorption_coeff[3];
} rtg_material_desc;

typedef struct rtg_texture_desc {    /* src/Texture.h:13-51 */
    int32_t kind;            /* rtg_texture_kind */
    int32_t decal;           /* rtg_decal_mode */
    int32_t interp;          /* rtg_interp */
    int32_t noise_conv;      /* rtg_noise_conv (Perlin) */
    int32_t normalizer;
    float noise_scale;
    float bump_factor;
    int32_t width;           /* image textures: texels is width*height*3 floats, */
    int32_t height;          /* row j=0 first, [j][i][c] — the values GetColorAtPixel returns */
    const float* texels;     /* (raw 0..255 for PNG/JPG, linear floats for EXR). */
} rtg_texture_desc;

typedef struct rtg_light_desc {      /* src/Light.h:35-139 */
    int32_t type;            /* rtg_light_type */
    float position[3];       /* point/spot/area */
    float direction[3];      /* directional/spot direction; area normal (normalized by the library) */
    float intensity[3];      /* point/spot intensity; directional/area radiance */
    float coverage_deg;      /* spot CoverageAngle */
    float falloff_deg;       /* spot FalloffAngle */
    float size;              /* area Size */
    int32_t texture;         /* environment: 0-based index into rtg_scene_desc.textures
                                (a bilinear, normalizer-1 image texture) */
} rtg_light_desc;

typedef struct rtg_scene_desc {
    int32_t abi_version;     /* RTG_ABI_VERSION */
    int32_t max_recursion_depth;   /* src/Parser.h:23 default 1 */
    float shadow_ray_eps;          /* default 0.002 */
    float intersection_test_eps;   /* default 0.001 */
    float background[3];
    float ambient_light[3];
    int32_t background_texture;    /* 0-based texture index with decal replace_background, -1 none
                                      (last such texture, src/Scene.cpp:494-500) */
    int32_t environment_light;     /* 0-based light index, -1 none (src/Parser.h:1302-1313) */

    const float* vertices;   int32_t num_vertices;    /* xyz triples */
    const float* texcoords;  int32_t num_texcoords;   /* uv pairs */
    const int32_t* faces;    int32_t num_faces;       /* mesh face triples (1-based vertex idx) */
    const float* translations; int32_t num_translations;  /* xyz */
    const float* scalings;   int32_t num_scalings;        /* xyz */
    const float* rotations;  int32_t num_rotations;       /* angle_deg, x, y, z */
    const float* composites; int32_t num_composites;      /* 16 floats, glm column-major m[col][row] */
    const rtg_xform_ref* xform_refs; int32_t num_xform_refs;
    const rtg_object_desc* objects;  int32_t num_objects;  /* order: spheres, triangles, meshes */
    const rtg_instance_desc* instances; int32_t num_instances;
    const rtg_material_desc* materials; int32_t num_materials;
    const rtg_texture_desc* textures;   int32_t num_textures;
    const rtg_light_desc* lights;       int32_t num_lights;
} rtg_scene_desc;

typedef struct rtg_camera_desc {     /* src/Camera.h:19-67; FovY/GazePoint already resolved */
    float position[3];
    float gaze[3];
    float up[3];
    float left, right, bottom, top;  /* near plane */
    float near_distance;
    int32_t nx, ny;
    int32_t num_samples;
    int32_t is_dof;                  /* FocusDistance present */
    float focus_distance;
    float aperture_size;
    int32_t left_handed;
    /* hw7 <Renderer> / <RendererParams> (pages/Page7.md:15-33, 41-45; no reference code) */
    int32_t integrator;              /* rtg_integrator */
    int32_t pt_flags;                /* rtg_pt_flags (path tracing only) */
} rtg_camera_desc;

typedef enum rtg_integrator {
    RTG_INTEGRATOR_REFERENCE = 0,    /* Scene::RecursiveShading (Whitted / distribution ray tracing) */
    RTG_INTEGRATOR_PATH = 1          /* hw7 path tracer */
} rtg_integrator;
typedef enum rtg_pt_flags {
    RTG_PT_IMPORTANCE = 1,           /* cosine-weighted hemisphere sampling (else uniform) */
    RTG_PT_NEE = 2,                  /* next event estimation towards object lights */
    RTG_PT_RUSSIAN_ROULETTE = 4      /* cosine-based termination, no MaxRecursionDepth cap */
} rtg_pt_flags;
#define RTG_PT_MAX_BOUNCES 32        /* hard cap on path length with Russian roulette */

typedef struct rtg_render_opts {
    uint64_t seed;           /* Philox key for all stochastic draws (reference: random_device) */
    int32_t row_offset;      /* render only rows y with (y / row_block) % row_stride == row_offset; */
    int32_t row_stride;      /* other rows are written as 0 (multi-GPU pixel sharding). 0/1 = all */
    int32_t traversal;       /* 0 = ordered + pruned (default), 1 = exhaustive (literal line test) */
    int32_t max_batch_rays;  /* 0 = auto */
    int32_t collect_stats;   /* 1 = count BVH node visits / triangle tests (slower) */
    int32_t collect_timing;  /* 1 = HIP-event time every closest-hit / shadow launch */
    int32_t streams;         /* passes in flight on separate HIP streams (0 = library default, 8) */
    int32_t row_block;       /* rows per shard interleave block (0/1 = single rows; the pass's pixel
                                tiles become (64/b) x b for b = 1, 2, 4, so they stay image-contiguous) */
    int32_t compact_rows;    /* 1: the output holds only the owned rows, in image order
                                (rows_owned*nx*3 floats; rows_owned = rtg_shard_rows()), for a
                                gather of the shards instead of a full-frame reduce */
    /* In-process multi-GPU fan-out (rtg_render / rtg_render_device; SURVEY.md §8(b) Threading,
       the GPU counterpart of the 8 std::threads of renderScene, src/Scene.cpp:294-363).  0/1: the
       scene's device only.  N > 1: the frame is cut into N shards of row blocks (row_block, 0 = 4;
       shard r owns the rows with (y / row_block) % N == r), one host thread per device renders
       one shard on a replica of the scene (device-to-device copies of the scene's buffers), and
       the shards' rows are gathered onto the scene's device with RCCL point-to-point transfers
       (ncclCommInitAll over the devices; librccl.so.1 is loaded on first use).  row_offset /
       row_stride / compact_rows must be 0. */
    int32_t num_devices;
    const int32_t* devices;  /* NULL: the scene's device followed by the next num_devices-1 device
                                indices (mod rtg_device_count()); else num_devices indices, devices[0]
                                = the scene's device.  A device listed twice takes no RCCL
                                communicator: its shard is copied with hipMemcpyPeer (rehearsal of
                                the N-shard path on fewer GPUs; results are identical). */
    /* ABI 7: ray scheduling.  RTG_SCHEDULE_AUTO: the stream schedule where built (the path
       tracer), else passes.  RTG_SCHEDULE_PASSES: every level of every pass is one launch.
       RTG_SCHEDULE_STREAM: steps that carry the survivors of any level together with new camera
       samples (DESIGN.md §4 "Schedules"); max_batch_rays then caps the rays of one step.  Results
       are bit-identical either way. */
    int32_t schedule;
    /* ABI 8 (these replace the environment knobs of earlier builds; 0 = the library default) */
    int32_t tile_band;       /* pixel order: bands this many 64-pixel tiles high, walked in columns of
                                tiles (0 = 64 owned rows: 8 tiles of 8 rows, 16 of a row shard's 4;
                                DESIGN.md §5).  Results do not depend on it. */
    int32_t segment_pixels;  /* stream schedule, path tracer: pixels whose samples' radiance is buffered
                                per segment (0 = as many as an eighth of the device memory holds) */
    int32_t segment_nodes;   /* stream schedule, reference integrator: a segment takes no new samples
                                once its node records exceed this many (0 = a quarter of the device
                                memory's worth).  Results do not depend on either. */
    int32_t pad_abi8;
} rtg_render_opts;
#define RTG_SCHEDULE_AUTO 0
#define RTG_SCHEDULE_PASSES 1
#define RTG_SCHEDULE_STREAM 2

/* Automatic pass size (rays per pass) of a render: at most 24M rays, lowered so that the level
   buffers of `lanes` passes in flight fit half of `device_bytes` (0 = no memory limit), at 2 x
   (228 + 68 x max(num_lights - 1, 0)) bytes per ray [+ 96 for the path tracer]; at least 64K. */
int64_t rtg_pass_rays(int32_t num_lights, int32_t path_tracer, int32_t lanes, uint64_t device_bytes);

/* Number of image rows y < ny with (y / row_block) % row_stride == row_offset. */
int32_t rtg_shard_rows(int32_t ny, int32_t row_offset, int32_t row_stride, int32_t row_block);

typedef struct rtg_render_stats {
    uint64_t primary_rays;
    uint64_t secondary_rays;
    uint64_t shadow_rays;
    uint64_t total_rays;
    double render_ms;        /* device time of the last rtg_render* call */
    int32_t passes;
    int32_t max_level;
    uint64_t node_visits;    /* collect_stats: 32-byte BVH child records read by closest-hit rays */
    uint64_t tri_tests;      /* collect_stats: triangle tests by closest-hit (primary+secondary) rays */
    uint64_t shadow_node_visits;   /* same for shadow queries */
    uint64_t shadow_tri_tests;
    double trace_ms;         /* collect_timing: summed device time of closest-hit launches */
    double shadow_ms;        /* collect_timing: summed device time of shadow launches */
    int32_t trace_launches;
    int32_t shadow_launches;
    uint64_t trace_steps;          /* collect_stats: BVH node steps (loop iterations) of closest-hit rays */
    uint64_t shadow_steps;
    uint64_t trace_lane_slots;     /* collect_stats: sum over waves of 64 x the wave's longest walk */
    uint64_t shadow_lane_slots;    /*   (SIMD efficiency = trace_steps / trace_lane_slots) */
    double shade_ms;         /* collect_timing: summed device time of the shading launches */
    int32_t shade_launches;
    int32_t devices;         /* devices that rendered the frame (num_devices fan-out or ranks: 1 here) */
    double gather_ms;        /* multi-GPU: host wall time from the last shard's end to the gathered frame */
    uint64_t shadow_blocked;       /* collect_stats: shadow queries found blocked ... */
    uint64_t shadow_blocked_steps; /*   ... their node steps and triangle tests (the remainder of */
    uint64_t shadow_blocked_tris;  /*   shadow_steps / shadow_tri_tests belongs to unblocked queries) */
    double resolve_ms;       /* collect_timing: summed device time of the bottom-up resolve launches */
    double accumulate_ms;    /* collect_timing: summed device time of the sample accumulation launches */
    int32_t resolve_launches;
    int32_t accumulate_launches;
    /* ABI 7, collect_stats: top-level entries (objects / instances) visited by the lanes -- the
       entry-start work of BVHMethods::FindIntersection's object loop (src/Helper.cpp:33-73): ray
       transform, root test, flat meshes' triangles -- and 64 x the entries each wave's loop went
       through.  (steps + entry_visits) / (lane_slots + entry_slots) is the SIMD efficiency with the
       object loop included. */
    uint64_t trace_entry_visits;
    uint64_t trace_entry_slots;
    uint64_t shadow_entry_visits;
    uint64_t shadow_entry_slots;
    /* ABI 7, collect_stats: blocked shadow queries (Light::IsShadow needs the nearest blocker,
       src/Light.cpp:188-204): histograms of the node steps taken before the eventual blocker was
       accepted (finding it) and after (proving it nearest), bins 0, 1, 2, 3-4, 5-8, 9-16, 17-32,
       > 32; and the steps before, summed */
    uint64_t shadow_hist_before[8];
    uint64_t shadow_hist_after[8];
    uint64_t shadow_blocked_steps_before;
    /* ... and the same sum with each blocked query's steps before replaced by the fewest any blocked
       query of its wave took (what sharing the first blocker found in a wave could save at most) */
    uint64_t shadow_blocked_steps_before_wavemin;
    /* ABI 8, collect_stats: wave cycles (shader clock, s_memtime, summed over waves) spent in each
       top-level entry of the linear object loop (entry-box test, ray transform, walk), closest-hit
       and shadow kernels; entries >= 15 share the last slot.  Where the traversal time goes per entry. */
    uint64_t trace_entry_cycles[16];
    uint64_t shadow_entry_cycles[16];
    /* ABI 8, collect_stats: path-tracer shading (k_pt_shade) wave cycles by phase -- hit set-up
       (ray, hit record), next-event estimation (light samples + BRDF), continuation sampling,
       compaction + record stores */
    uint64_t pt_shade_cycles[4];
    /* ABI 9, collect_stats: the flat group (untransformed small meshes tested together):
       the (lane, triangle) tests its lanes ran -- every member triangle's fast rejection, then each lane's
       own candidates' exact tests -- and 64 x the tests each wave ran (the most any of its lanes needed).
       (steps + entry_visits + group_work) / (lane_slots + entry_slots + group_slots) is the SIMD
       efficiency with the group's per-lane work counted.  group_cycles: the group's wave cycles split
       into set-up (ray transform, reciprocals, window) and tests (slot 15 of entry_cycles holds both). */
    uint64_t trace_group_work;
    uint64_t trace_group_slots;
    uint64_t shadow_group_work;
    uint64_t shadow_group_slots;
    uint64_t trace_group_cycles[2];
    uint64_t shadow_group_cycles[2];
} rtg_render_stats;

typedef struct rtg_ray {             /* src/Ray.h:10-12 */
    float origin[3];
    float direction[3];
    float time;
} rtg_ray;

typedef struct rtg_hit {             /* what FindIntersection leaves in ReturnVal for a hit */
    int32_t full;            /* 1 = hit */
    int32_t object;          /* top-level index: [0,num_objects) objects, then instances */
    int32_t prim;            /* primitive index in the object's original (parse) order */
    int32_t material;        /* 1-based material (instance override applied) */
    float t;                 /* gett() distance along the world ray (src/Helper.cpp:41) */
    float point[3];          /* world hit point = ray.getPoint(t) */
    float normal[3];         /* world normal after TransformNormal (src/Helper.cpp:75-77) */
} rtg_hit;

typedef struct rtg_scene rtg_scene;

int32_t rtg_abi_version(void);
const char* rtg_last_error(void);
int32_t rtg_device_count(void);

#define RTG_DEVICE_HOST_ONLY (-1)
/* Build device-resident scene on HIP device `device`.  RTG_DEVICE_HOST_ONLY builds only
   the host-side structures (matrices, normals, BVH) for introspection; such a scene
   cannot render or trace (RTG_ERR_NO_DEVICE). */
int32_t rtg_scene_create(const rtg_scene_desc* desc, int32_t device, rtg_scene** out);

/* BVH builder selection for rtg_scene_create_ex.  All builders produce the reference's tree
   (src/BVH.cpp:64-135) bit for bit; they differ only in where the work runs. */
typedef enum rtg_bvh_builder {
    RTG_BVH_AUTO = 0,   /* GPU for meshes of >= 4096 finite triangles on a device scene, else host
                           (the SAH traversal tree: GPU from 65536 triangles) */
    RTG_BVH_HOST = 1,   /* recursive host build */
    RTG_BVH_GPU = 2     /* level-synchronous GPU build (falls back to host for non-finite input) */
} rtg_bvh_builder;
typedef struct rtg_build_opts {
    int32_t bvh_builder;     /* rtg_bvh_builder */
    int32_t tlas;            /* top-level BVH over objects and instances, replacing the reference's
                                linear object loop (src/Helper.cpp:32-73) with the same result (ties
                                to the first entry): 0 = auto (>= 16 entries), 1 = off, 2 = on
                                (>= 2 entries) */
    int32_t traversal_tree;  /* 0 = fast rays walk an SAH 4-wide tree per mesh (candidates checked for
                                reachability in the reference tree, ties in its order: same results);
                                1 = the reference tree only */
    /* ABI 8: 0 = waves of camera samples and of their shadow queries walk the traversal tree
       together (wave-uniform node loads); 1 = every lane walks alone.  Same results. */
    int32_t uniform_walk;
} rtg_build_opts;
/* rtg_scene_create with build options (NULL = defaults). */
int32_t rtg_scene_create_ex(const rtg_scene_desc* desc, int32_t device, const rtg_build_opts* opts,
                            rtg_scene** out);
typedef struct rtg_build_stats {
    double bvh_build_ms;     /* wall time of all per-object BVH constructions */
    int32_t bvh_gpu_objects; /* objects whose BVH was built on the GPU */
    int32_t num_objects;
    int32_t tlas_nodes;      /* nodes of the top-level BVH (0: linear object loop) */
    int32_t flat_group_entries;  /* ABI 8: entries in the flat group (closest_hit) */
    /* ABI 7: wall-time split of rtg_scene_create (ms), in build order.  Together they cover the
       whole call (total_ms); the reference does this work at the start of renderScene
       (src/Scene.cpp:296-323, BVH.cpp:53-62). */
    double validate_ms;      /* descriptor checks (every face index) */
    double prep_ms;          /* vertices, per-object primitive lists, matrices, smooth normals */
    double median_tree_ms;   /* the reference's median-split trees (= bvh_build_ms) */
    double records_ms;       /* triangle records, reference-node flattening, reachability gates */
    double traversal_tree_ms;/* the SAH 4-wide traversal trees (build + collapse) */
    double top_level_ms;     /* entries, world boxes, top-level BVH, materials, textures, lights */
    double upload_ms;        /* host -> device copies of every scene buffer */
    double total_ms;         /* the whole rtg_scene_create call */
    uint64_t upload_bytes;   /* bytes copied to the device */
    /* ABI 8: traversal trees (SAH) built on the GPU (rtg_bvh_builder applies to both trees), their
       binary nodes before the 4-wide collapse, and an order-independent hash of those nodes (box and
       triangle count of every node): the host and GPU builds of a mesh give the same hash unless a
       range with all centroids equal was halved by count */
    int32_t sah_gpu_objects;
    int32_t pad_abi8;
    uint64_t traversal_nodes;
    uint64_t traversal_hash;
} rtg_build_stats;
int32_t rtg_scene_build_stats(const rtg_scene* scene, rtg_build_stats* out);
int32_t rtg_scene_destroy(rtg_scene* scene);

/* Render one camera; rgb_out is caller-owned host memory of ny*nx*3 floats ([y][x][c])
   (rows_owned*nx*3 with opts->compact_rows). */
int32_t rtg_render(rtg_scene* scene, const rtg_camera_desc* cam, const rtg_render_opts* opts,
                   float* rgb_out);
/* Same, output left in device memory (caller-owned, ny*nx*3 floats on the scene's device),
   enqueued on `stream` (hipStream_t, NULL = default stream). Synchronous on return. */
int32_t rtg_render_device(rtg_scene* scene, const rtg_camera_desc* cam,
                          const rtg_render_opts* opts, float* rgb_out_device, void* stream);
int32_t rtg_last_render_stats(const rtg_scene* scene, rtg_render_stats* out);

/* ---- multi-process multi-GPU (one process per GPU) ------------------------
   The same shard + RCCL gather as rtg_render_opts.num_devices, for callers that run one process
   (rank) per GPU, e.g. under torch.distributed.run: rank 0 makes an id with rtg_comm_unique_id,
   hands the RTG_COMM_ID_BYTES bytes to every rank (any side channel), and each rank calls
   rtg_comm_init_rank (ncclCommInitRank).  rtg_render_ranked renders this rank's row-block shard
   (row_offset = rank, row_stride = nranks, row_block = opts->row_block or 4) and gathers the
   shards' rows into `frame_device` (ny*nx*3 floats on rank 0's device; may be NULL on other
   ranks).  Every rank must call it for the same camera.  Synchronous on return. */
#define RTG_COMM_ID_BYTES 128
typedef struct rtg_comm rtg_comm;
int32_t rtg_comm_unique_id(uint8_t id[RTG_COMM_ID_BYTES]);
int32_t rtg_comm_init_rank(const uint8_t id[RTG_COMM_ID_BYTES], int32_t nranks, int32_t rank, int32_t device,
                           rtg_comm** out);
/* ABI 8: the same with a bound on every wait of the rank (communicator set-up, the failure agreement
   and the gather of rtg_render_ranked): a rank whose peers do not join within timeout_ms aborts the
   communicator (ncclCommAbort) and returns RTG_ERR_HIP instead of blocking; the communicator is then
   unusable (destroy it).  The agreement / gather deadline counts from this rank's own shard end, so it
   must also cover the peers' remaining render time (shard skew).  timeout_ms <= 0: no deadline, which is
   what rtg_comm_init_rank does (round 6, ADVICE r5: a long, imbalanced render must not abort a healthy
   rank). */
int32_t rtg_comm_init_rank_timeout(const uint8_t id[RTG_COMM_ID_BYTES], int32_t nranks, int32_t rank, int32_t device,
                                   int32_t timeout_ms, rtg_comm** out);
int32_t rtg_comm_destroy(rtg_comm* comm);
int32_t rtg_render_ranked(rtg_scene* scene, const rtg_camera_desc* cam, const rtg_render_opts* opts, rtg_comm* comm,
                          float* frame_device, void* stream);

/* hw5 tone mapping (pages/Page5.md:47-53 describes a global operator; src/ has none): the
   Photographic TMO of DESIGN.md §11, from a camera's <Tonemap> (<TMO>Photographic</TMO>
   <TMOOptions>key burn%</TMOOptions> <Saturation> <Gamma>).  Output: 0..255 floats, [y][x][c]. */
typedef enum rtg_tmo { RTG_TMO_PHOTOGRAPHIC = 0 } rtg_tmo;
typedef struct rtg_tonemap_desc {
    int32_t tmo;             /* rtg_tmo */
    float key;               /* TMOOptions[0], e.g. 0.18 */
    float burn_percent;      /* TMOOptions[1]: percentage of the brightest pixels that saturate */
    float saturation;
    float gamma;
} rtg_tonemap_desc;
/* hdr_rgb / ldr_rgb: host arrays of ny*nx*3 floats; the work runs on HIP device `device`. */
int32_t rtg_tonemap(int32_t device, const float* hdr_rgb, int32_t nx, int32_t ny, const rtg_tonemap_desc* tm,
                    float* ldr_rgb);
/* Same on device arrays, enqueued on `stream` (hipStream_t); synchronous on return. */
int32_t rtg_tonemap_device(int32_t device, const float* hdr_rgb_device, int32_t nx, int32_t ny,
                           const rtg_tonemap_desc* tm, float* ldr_rgb_device, void* stream);

/* Batch closest-hit query (BVHMethods::FindIntersection) over host arrays. */
int32_t rtg_trace_closest(rtg_scene* scene, const rtg_ray* rays, int32_t n, rtg_hit* hits,
                          int32_t traversal);

/* Introspection for BVH parity tests: per object (0-based, objects only).
   perm[k] = original primitive index at BVH position k (length num_prims).
   nodes: num_nodes * 4 int32 {left, right, start, end} in the reference's pre-order
   (node, left subtree, right subtree); left/right are node numbers or -1 (null),
   start/end is the primitive range the node covers; leaves have left=right=-1.
   boxes: num_nodes * 6 floats (min xyz, max xyz; leaves hold the leaf's own range box,
   which the reference never tests).  Pass NULL buffers to query the sizes. */
int32_t rtg_scene_object_bvh(const rtg_scene* scene, int32_t object, int32_t* num_prims,
                             int32_t* num_nodes, int32_t* perm, int32_t* nodes, float* boxes);
/* Composed matrices per top-level object (objects then instances): inverse and
   inverse-transpose, glm column-major, 16 floats each. */
int32_t rtg_scene_object_matrices(const rtg_scene* scene, int32_t top_object, float* inverse16,
                                  float* inverse_transpose16);
/* Smooth vertex normals after the precompute of renderScene (src/Scene.cpp:294-318): 3*num_vertices. */
int32_t rtg_scene_vertex_normals(const rtg_scene* scene, float* normals);

/* ---- ABI 10: resumable progressive frames -----------------------------------
   An rtg_frame is a device-resident accumulator for one camera of one scene: the running float32
   sum of every owned pixel's samples, in sample order, and optionally the running mean and M2
   (Welford) of the samples' luminance.  Samples are added in index order, first_sample + done,
   + 1, ...; sample k of a pixel is the same ray tree whichever call traces it (every random draw
   is keyed by pixel and global sample index), and the sum continues ((s + c_k) + c_k+1) + ... as
   one rtg_render does, so a frame over [0, num_samples) resolves, after any chunking, to exactly
   what rtg_render returns for the same camera and options -- on either schedule.
   The camera, seed, shard options (row_offset / row_stride / row_block / compact_rows), traversal,
   schedule and batch options are fixed at creation.  num_devices > 1 or devices != NULL:
   RTG_ERR_UNSUPPORTED.  The accumulator is the frame's own (12 B per owned pixel, + 8 B with
   moments); the render workspace is the scene's, so calls on one scene must not be concurrent, but
   frames and rtg_render calls may interleave.  rtg_scene_destroy fails with RTG_ERR_INVALID while
   a scene has live frames. */
typedef struct rtg_frame rtg_frame;
typedef struct rtg_frame_opts {
    int32_t first_sample;    /* first index of the camera's num_samples that this frame covers */
    int32_t sample_count;    /* how many it covers; 0 = through the last one */
    int32_t moments;         /* 1: keep a running mean and M2 of each pixel's sample luminance */
    int32_t order;           /* sample order (ABI 10 additions below): 0 = index order, 1 = spread */
} rtg_frame_opts;
/* Error estimate over the owned pixels.  Y = (0.2126 R + 0.7152 G) + 0.0722 B of a sample, 0 when
   negative or not finite; per pixel, variance = M2 / (n - 1) (0 for n < 2) and the standard error
   of the mean sem = sqrt(variance / n), n = samples_done. */
typedef struct rtg_frame_error {
    double mean_luminance;   /* mean over the pixels of the per-pixel mean of Y */
    double mean_sem;         /* mean over the pixels of sem */
    double max_sem;
    int32_t samples_done;
    int32_t pixels;          /* owned pixels */
} rtg_frame_error;
/* opts / fopts may be NULL (defaults: seed 0, the whole camera, no moments). */
int32_t rtg_frame_create(rtg_scene* scene, const rtg_camera_desc* cam, const rtg_render_opts* opts,
                         const rtg_frame_opts* fopts, rtg_frame** out);
/* Trace the next `count` samples of every owned pixel (work enqueued behind `stream`, a hipStream_t;
   synchronous on return).  rtg_last_render_stats then describes this call alone. */
int32_t rtg_frame_add_samples(rtg_frame* frame, int32_t count, void* stream);
/* Samples accumulated so far (negative status for a NULL frame). */
int32_t rtg_frame_samples_done(const rtg_frame* frame);
/* sum / (float)samples_done for owned pixels, 0 for the others; layout as rtg_render (host) and
   rtg_render_device. */
int32_t rtg_frame_resolve(rtg_frame* frame, float* rgb_out);
int32_t rtg_frame_resolve_device(rtg_frame* frame, float* rgb_out_device, void* stream);
/* Per owned pixel, in owned-row order (rows_owned * nx floats each; either may be NULL): the mean
   and the unbiased variance of the samples' luminance. */
int32_t rtg_frame_moments(rtg_frame* frame, float* mean_out, float* variance_out);
int32_t rtg_frame_error_stats(rtg_frame* frame, rtg_frame_error* out);
/* Checkpoint: the raw sums (3 floats per owned pixel) and, for a frame with moments, mean and M2
   (2 per owned pixel), to and from host memory.  A state restored into a frame of the same camera,
   options and window -- of this scene or of another built from the same descriptor -- and continued
   finishes bit-identical to an uninterrupted frame.  moments_out may be NULL; sums / moments may be
   NULL when samples_done is 0. */
int32_t rtg_frame_get_state(rtg_frame* frame, float* sums_out, float* moments_out);
int32_t rtg_frame_set_state(rtg_frame* frame, int32_t samples_done, const float* sums, const float* moments);
int32_t rtg_frame_destroy(rtg_frame* frame);

/* ---- ABI 10 additions: adaptive sampling ------------------------------------
   Additive: the version stays 10, no struct grows (rtg_frame_opts.order was its pad).

   Sample order.  The camera's samples are stratified row by row (sample k sits in cell (k mod g,
   k / g) of a g x g grid), so a prefix in index order covers the first sub-pixel rows only.  With
   order 1, position j of a frame traces sample (j * m) mod n, n = num_samples: m = 1 for n <= 2,
   else the smallest m >= max(1, (n * 618034 + 500000) / 1000000) (64-bit integers) with
   gcd(m, n) = 1 -- a bijection of [0, n) whose prefixes are spread over the pixel.  first_sample,
   sample_count and samples_done then count positions.  Sample k itself is the same ray tree (jitter
   cell and random draws are keyed by pixel and sample index); the sums and the moments run in
   position order, so an order-1 frame equals the same samples summed in that order, not rtg_render
   bit for bit.  n > 32768 with order 1: RTG_ERR_UNSUPPORTED; an order other than 0 / 1: RTG_ERR_INVALID.
   rtg_sample_order_index returns the sample index of `position` (negative status on bad arguments).

   Retirement.  A pixel of a frame is active or retired; retirement is monotone (only
   rtg_frame_set_state, which makes every pixel active again, and rtg_frame_set_retired undo it).
   Every active pixel holds exactly samples_done samples; a retired pixel keeps the count it had when
   it was retired.  rtg_frame_add_samples traces the next `count` positions of the active pixels
   only (rtg_last_render_stats.primary_rays = active x count; no active pixel: nothing is traced,
   RTG_OK) and advances samples_done.  resolve divides each pixel by its own count (0 samples: 0),
   rtg_frame_moments and rtg_frame_error_stats use each pixel's own n (rtg_frame_error.samples_done
   stays the frame's).  get_state / set_state are unchanged: the counts and flags travel through
   rtg_frame_sample_counts / rtg_frame_set_retired.  Storage: 4 B per owned pixel for count and flag
   and 4 B for the active list, allocated by the first retirement; a frame that never retires
   allocates nothing and launches what it did before. */
typedef struct rtg_frame_adapt {
    float rel_tol;           /* retire when sem <= max(abs_tol, rel_tol * mean luminance) ... */
    float abs_tol;
    int32_t min_samples;     /* ... and samples_done >= max(min_samples, 2) */
    int32_t pad;
} rtg_frame_adapt;
int32_t rtg_sample_order_index(int32_t num_samples, int32_t order, int32_t position);
/* Needs moments and samples_done >= 1.  Retires every active pixel with n = samples_done >=
   max(min_samples, 2) and (double)var / (double)n <= thr * thr, var = M2 / (float)(n - 1) in float32
   as rtg_frame_moments returns it, thr = fmax((double)abs_tol, (double)rel_tol * (double)mean) --
   squared on purpose: no sqrt, so a float64 restatement decides identically.  Negative or non-finite
   tolerances: RTG_ERR_INVALID.  *active_out (may be NULL): the active pixels left. */
int32_t rtg_frame_retire(rtg_frame* frame, const rtg_frame_adapt* adapt, int32_t* active_out);
/* Retires the active pixels whose byte of `retire` (host, rows_owned * nx, owned-row order) is not 0;
   with or without moments, and also at samples_done == 0 (a region-of-interest render: a pixel
   retired without samples resolves to 0). */
int32_t rtg_frame_retire_mask(rtg_frame* frame, const uint8_t* retire, int32_t* active_out);
int32_t rtg_frame_active_pixels(const rtg_frame* frame);
/* Per owned pixel, owned-row order: the samples it holds and 1 / 0 for retired / active; either may
   be NULL. */
int32_t rtg_frame_sample_counts(rtg_frame* frame, int32_t* counts_out, uint8_t* retired_out);
/* Restores counts and flags after rtg_frame_set_state: 0 <= counts[p] <= samples_done, and
   counts[p] == samples_done for every pixel that is not retired. */
int32_t rtg_frame_set_retired(rtg_frame* frame, const int32_t* counts, const uint8_t* retired);

/* ---- ABI 10 additions: first-hit feature buffers and camera rays -------------
   Additive: the version stays 10, no struct grows.

   rtg_render_aov: per owned pixel, over a window of the camera's samples, what the primary rays hit
   first -- the inputs of a denoiser, a compositor or an id picker.  Sample k of a pixel is the primary
   ray rtg_render traces for it under opts->seed (a one-sample camera keeps its pixel-centre ray).  The
   window's samples are visited in index order; for a sample that hits, t is the rtg_hit.t and n the
   rtg_hit.normal (the shading normal: after bump / replace-normal textures and the object's transform)
   that rtg_trace_closest reports for that ray, and a the diffuse reflectance its shading would use, by
   the hit's decal mode: replace_kd / replace_all: tc / tn; blend_kd: (kd + tc / tn) * 0.5f; else kd
   (kd: the material's diffuse, instance override applied; tc, tn: texture colour and normalizer;
   component-wise float32).  depth, normal and albedo each start at +0, add t, n, a of the hit samples
   in window order and divide by (float)hits; 0 where hits == 0.  normal is not renormalised.  ids
   describe the window's FIRST sample alone: (top-level object, primitive in parse order as
   rtg_hit.prim, 1-based material), or (-1, -1, 0) for a miss.
   Layout and ownership are rtg_render's: [y][x][c], rows the shard does not own written as 0 (ids:
   -1, -1, 0); with compact_rows only the owned rows.  seed, row_offset, row_stride, row_block,
   compact_rows and traversal are honoured; the other option fields, the camera's integrator and its
   pt_flags do not change the result.  num_devices > 1 or devices != NULL: RTG_ERR_UNSUPPORTED.
   rtg_last_render_stats then reports primary_rays = total_rays = owned pixels x window and the device
   time in render_ms.  The call may interleave with renders and frames on the scene (never run
   concurrently with them) and leaves a live frame's accumulator untouched.  opts / aov may be NULL
   (seed 0, the whole camera). */
typedef struct rtg_aov_opts {      /* 16 bytes */
    int32_t first_sample;          /* window of the camera's num_samples, in index order */
    int32_t sample_count;          /* 0 = through the last sample */
    int32_t pad[2];                /* must be 0 */
} rtg_aov_opts;
typedef struct rtg_aov_buffers {   /* host pointers; each may be NULL, not all */
    int32_t* hits;    /* 1 per pixel: samples of the window whose primary ray hit */
    float*   depth;   /* 1 per pixel */
    float*   normal;  /* 3 per pixel */
    float*   albedo;  /* 3 per pixel */
    int32_t* ids;     /* 3 per pixel: object, prim, material of the window's FIRST sample */
} rtg_aov_buffers;
int32_t rtg_render_aov(rtg_scene* scene, const rtg_camera_desc* cam, const rtg_render_opts* opts,
                       const rtg_aov_opts* aov, const rtg_aov_buffers* out);
/* The camera's primary rays for every pixel of the whole image (no sharding), as the renderer forms them
   under `seed`: rays_out[(y * nx + x) * count + j] is sample first_sample + j (count = sample_count, or
   num_samples - first_sample for 0): origin, direction and time (0 for a one-sample or depth-of-field
   camera).  Computed on the scene's device.  Ready for rtg_trace_closest. */
int32_t rtg_camera_rays(rtg_scene* scene, const rtg_camera_desc* cam, uint64_t seed, int32_t first_sample,
                        int32_t sample_count, rtg_ray* rays_out);

/* ---- ABI 10 additions: an edge-avoiding denoiser for frames -------------------
   Additive: the version stays 10, no struct grows.

   rtg_denoise: an a-trous (dilated 5x5 B3-spline) wavelet filter over an image, stopped at edges of the
   first-hit normal, of the depth (with a per-pixel slope) and, where a variance is given, of the
   luminance (with a width in standard deviations of the 3x3-filtered variance).  With an albedo the
   image is divided by max(albedo, 1/256) first and multiplied back afterwards, so texture detail is not
   blurred.  A pixel is valid when its depth is finite and > 0 and its rgb and normal are finite; an
   invalid pixel comes back as it went in, bit for bit, and feeds no other pixel.  A variance that is
   negative or not finite counts as 0.  Float32 in a fixed order, no atomics: results repeat bit for
   bit (the exact arithmetic: DESIGN.md §18).  Arguments are checked before the device is touched.
   rgb_out may not alias an input. */
typedef struct rtg_denoise_opts {   /* 32 bytes; NULL = all defaults */
    int32_t iterations;         /* 0 = 5; 1..8; iteration i uses tap stride 2^i */
    float   sigma_l;            /* 0 = 4.0f; luminance stop width in standard deviations */
    float   sigma_z;            /* 0 = 1.0f; depth stop width in per-pixel slopes */
    int32_t normal_power_log2;  /* 0 = 6 (power 64); 1..10: the normal stop is squared this many times */
    int32_t pad[4];             /* must be 0 */
} rtg_denoise_opts;
typedef struct rtg_denoise_inputs { /* 40 bytes; ny*nx pixels each, [y][x][c] */
    const float* rgb;       /* 3 per pixel: the image to filter (0..255 scale, unclamped) */
    const float* normal;    /* 3 per pixel: rtg_render_aov's normal */
    const float* depth;     /* 1 per pixel: rtg_render_aov's depth; <= 0 or non-finite: no surface */
    const float* albedo;    /* 3 per pixel or NULL (no demodulation) */
    const float* variance;  /* 1 per pixel or NULL (no luminance stop): variance of the pixel's MEAN
                               luminance = rtg_frame_moments' variance / the pixel's sample count */
} rtg_denoise_inputs;
/* Host arrays; the work runs on HIP device `device`. */
int32_t rtg_denoise(int32_t device, const rtg_denoise_inputs* in, int32_t nx, int32_t ny,
                    const rtg_denoise_opts* opts, float* rgb_out);
/* Same on device arrays, enqueued on `stream` (hipStream_t); synchronous on return. */
int32_t rtg_denoise_device(int32_t device, const rtg_denoise_inputs* in_device, int32_t nx, int32_t ny,
                           const rtg_denoise_opts* opts, float* rgb_out_device, void* stream);

/* ---- ABI 10 additions: denoising a frame on the device ------------------------
   Additive: the version stays 10, no struct grows.

   rtg_frame_denoise filters the frame's current image without anything leaving the device: the image is
   rtg_frame_resolve's; normal, depth and albedo are rtg_render_aov's over the camera's whole sample range
   (first 0, count 0) under the frame's seed and traversal, tile_band 0 as rtg_render_aov sets it; the
   albedo is used only when demodulate != 0.  For a frame with moments and samples_done >= 2 the variance
   of each pixel's mean luminance opens the luminance stop: with n the pixel's own count (samples_done for
   an active pixel, the kept count for a retired one), (M2 / (float)(n - 1)) / (float)n for n >= 2 -- two
   correctly rounded float32 divides, rtg_frame_moments' variance over the float32 count -- and +0 for
   n < 2.  A frame without moments, or with one sample, runs without the luminance stop.  The result is,
   bit for bit, rtg_denoise over those arrays.  A frame window with first_sample > 0 and an order-1 frame
   are allowed (the guides still cover the camera's whole range).

   Checked before any device work, in this order: NULL frame or output (RTG_ERR_INVALID); a frame whose
   state a failed call lost, or without samples (RTG_ERR_INVALID); the options, by rtg_denoise's rules;
   a sharded frame (row_stride > 1) or a compact_rows frame (RTG_ERR_UNSUPPORTED).

   State.  The first of these calls on a frame allocates, and rtg_frame_destroy releases: the guide cache
   (normal, depth, albedo in image order, 28 B per pixel), traced once by that call and never again --
   the guides are a function of scene, camera, seed and traversal, all fixed at rtg_frame_create, so
   rtg_frame_set_state, rtg_frame_set_retired and further samples leave them valid; the call inputs
   (resolved rgb and variance, 16 B per pixel), rewritten by every call; the filter's workspace (56 B per
   pixel), kept between calls.  In all 100 B per pixel, about 207 MB at 1920x1080.  A frame that never
   denoises allocates nothing and launches what it did before.

   The call that traces the guides leaves rtg_last_render_stats as rtg_render_aov does (primary_rays =
   total_rays = pixels x num_samples); a later call leaves the scene's stats untouched.  Calls may
   interleave with renders, other frames and rtg_render_aov on the scene, never run concurrently with
   them; they change no bit of the accumulator, the moments or the counts.  The work is enqueued behind
   `stream` (hipStream_t); synchronous on return.  rgb_out_device must not alias the frame's own buffers
   (no call hands those out). */
typedef struct rtg_frame_guides {   /* 40 bytes; DEVICE pointers on the scene's device, each may be NULL, not all */
    float* rgb;       /* 3 per pixel: what rtg_frame_resolve_device writes */
    float* normal;    /* 3 per pixel */
    float* depth;     /* 1 per pixel */
    float* albedo;    /* 3 per pixel */
    float* variance;  /* 1 per pixel: variance of the pixel's MEAN luminance */
} rtg_frame_guides;
/* opts may be NULL (defaults); rgb_out: host, ny * nx * 3 floats. */
int32_t rtg_frame_denoise(rtg_frame* frame, const rtg_denoise_opts* opts, int32_t demodulate, float* rgb_out);
int32_t rtg_frame_denoise_device(rtg_frame* frame, const rtg_denoise_opts* opts, int32_t demodulate,
                                 float* rgb_out_device, void* stream);
/* Copies the five arrays the filter would read at the frame's current state into the caller's device
   arrays (refusals as above, without the options).  variance where the frame has none (no moments, or
   fewer than two samples): RTG_ERR_INVALID. */
int32_t rtg_frame_guides_device(rtg_frame* frame, const rtg_frame_guides* out_device, void* stream);

/* ---- ABI 10 additions: occlusion queries and ray queries on device arrays -----
   Additive: the version stays 10, no struct grows.

   rtg_trace_occluded answers "is anything in front of tmax?" for a batch of rays: occluded[i] = 1 iff
   rtg_trace_closest would report, for the same ray, time and scene, full != 0 and t < tmax[i] (t is
   rtg_hit.t: with an unnormalised direction both are in units of the ray parameter); else 0.  tmax NULL
   means +inf for every ray; a tmax that is NaN, zero or negative gives 0, and so does a ray with a NaN
   origin or direction.  traversal 0 (pruned) stops a ray at the first top-level entry that settles its
   answer; traversal 1 (exhaustive) runs the reference's whole loop and compares afterwards.  Both give
   the same bytes.

   The _device forms take device arrays on the scene's device -- rays as rtg_ray records (28 B), hits as
   rtg_hit records (44 B), one byte per ray for the occlusion -- and are enqueued on `stream`
   (hipStream_t); synchronous on return.  They copy nothing to the host.  Their workspace (the rays as
   planes and one 16-byte hit record per ray: 44 B per ray) is kept on the scene, grows to the largest n
   seen, is released by rtg_scene_destroy and is shared with no render, frame or feature-buffer call: a
   query between two renders or two rtg_frame_add_samples changes no bit of theirs.  Once it is large
   enough a call allocates nothing.  rtg_trace_occluded stages its host arrays in device memory for the
   call (33 B per ray) and uses the same workspace.  Two concurrent calls on one scene are as unsupported
   as two renders are.

   Checked in this order: NULL scene, n < 0, or a NULL rays / hits / occluded array with n > 0
   (RTG_ERR_INVALID); n == 0 (RTG_OK, nothing touched); a host-only scene (RTG_ERR_NO_DEVICE). */
int32_t rtg_trace_occluded(rtg_scene* scene, const rtg_ray* rays, const float* tmax, int32_t n,
                           uint8_t* occluded, int32_t traversal);
int32_t rtg_trace_closest_device(rtg_scene* scene, const rtg_ray* rays_device, int32_t n,
                                 rtg_hit* hits_device, int32_t traversal, void* stream);
int32_t rtg_trace_occluded_device(rtg_scene* scene, const rtg_ray* rays_device, const float* tmax_device,
                                  int32_t n, uint8_t* occluded_device, int32_t traversal, void* stream);

/* ---- ABI 10 additions: updating a built scene in place --------------------------
   Additive: the version stays 10, no struct grows.

   rtg_scene_update re-derives the top level of a built scene -- entries, world bounds, top-level BVH, flat
   group, materials, lights -- from a whole descriptor, without touching what was built per object (smooth
   normals, both trees of every mesh, the triangle records).  The descriptor has a frozen part, which must
   equal the build's, and a free part, which may change.

   Frozen: vertices, texcoords, faces, every texture's texels and every other field of the texture table;
   intersection_test_eps; per object type, id, center, radius, v, face_first, face_count, smooth,
   num_textures, textures, texture_offset, is_light, radiance; per instance base_object and id; num_objects,
   num_instances, num_vertices, num_texcoords, num_faces, num_textures, num_materials.  The frozen arrays
   (vertices, texcoords, faces, texels) may be NULL, meaning "as built": they are never read.
   Free: the four transformation tables and xform_refs with their counts; per object and instance
   xform_first, xform_count, blur, material, and an instance's reset_transform; materials; lights and
   num_lights (with the object lights at most 64); environment_light, background_texture, background,
   ambient_light, shadow_ray_eps, max_recursion_depth.

   After RTG_OK every call on the scene gives, bit for bit, what it gives on a scene freshly created on the
   same device with the same build options from the build's frozen part joined with desc's free part.
   Updates compose.  rtg_scene_build_stats then reports tlas_nodes, flat_group_entries, top_level_ms,
   upload_ms, upload_bytes and total_ms of the update alone; the other fields stay as built.

   Checked in this order, before anything is touched: NULL scene or desc (RTG_ERR_INVALID); a scene with
   live frames (RTG_ERR_INVALID: a frame's accumulator and cached guides belong to the scene it was made
   on); the descriptor checks of rtg_scene_create (RTG_ERR_INVALID); a changed frozen field
   (RTG_ERR_UNSUPPORTED, the message names it).  A failure after that leaves the scene unusable for
   everything but rtg_scene_destroy, and the message says so.  A host-only scene updates too.  Calls on one
   scene must not be concurrent. */
int32_t rtg_scene_update(rtg_scene* scene, const rtg_scene_desc* desc);
/* A 64-bit FNV-1a hash of the host images of everything the top-level phases produce, as uploaded (the
   arrays in a fixed order, then the scalars of the kernels' view: DESIGN.md §24), computed at the end of
   rtg_scene_create and rtg_scene_update; host-only scenes have it too.  Equal descriptors give equal
   hashes: an updated scene can be held against a fresh one without rendering. */
int32_t rtg_scene_top_hash(const rtg_scene* scene, uint64_t* out);

/* ---- ABI 10 additions: rendering caller-supplied primary rays -------------------
   Additive: the version stays 10, no struct grows.

   rtg_render_rays runs the integrator -- the reference's or the path tracer -- over primary rays the
   caller supplies: panoramas, fisheye and orthographic views, cube-map and probe captures, lightmap
   texels, any camera model.  rays[((size_t)y * nx + x) * num_samples + s] is sample s of pixel (x, y):
   rtg_camera_rays' layout with first_sample = 0.  Everything else is rtg_render's for a camera of the
   same nx, ny, num_samples, integrator and pt_flags: ray (pixel, s) takes the place of primary ray
   (pixel, s); every random draw below level 0 is keyed by pixel = y * nx + x and sample s under
   opts->seed; a miss takes the background of pixel (x, y), with the background texture's (row, col) rule
   and its transposition for num_samples == 1; a pixel's samples are summed in index order and divided as
   rtg_render divides; the output layout, the row shards (row_offset, row_stride, row_block, compact_rows),
   traversal, schedule, max_batch_rays, streams, tile_band, the segment options, collect_stats and
   collect_timing mean what they mean there.  So rendering a camera's own rays (rtg_camera_rays under the
   same seed) gives rtg_render's image bit for bit.  Directions are used as given, not normalised: supply
   unit directions (the reference's own rays are unit).

   rtg_last_render_stats then reports primary_rays = owned pixels x num_samples, the other fields as after
   rtg_render.  The call may interleave with renders, frames, feature buffers and queries on the scene
   (never run concurrently with them) and leaves a live frame untouched.  The _device form reads the
   caller's array on the scene's device in place and copies nothing; it is enqueued on `stream`
   (hipStream_t) and synchronous on return.  The host form stages the rays (28 B per ray) and the frame in
   device memory for the call and releases them.

   Checked in this order, all before anything is traced: a NULL scene, image, rays or output
   (RTG_ERR_INVALID); nx, ny or num_samples < 1, a non-zero pad, an unknown integrator or pt_flags bit
   (RTG_ERR_INVALID); the options, as rtg_render reports them; num_devices > 1 or devices != NULL
   (RTG_ERR_UNSUPPORTED: the rays live on one device); a host-only scene (RTG_ERR_NO_DEVICE); then, on the
   device, the rays the call will read (a shard: its owned rows only): a ray with a non-finite origin,
   direction or time, or with the direction (+-0, +-0, +-0), gives RTG_ERR_INVALID, the message naming the
   lowest such index, and the output is not written.

   Not offered: frames or feature buffers over caller rays, a CLI / XML surface, multi-device fan-out. */
typedef struct rtg_ray_image {   /* 32 bytes */
    int32_t nx, ny;              /* image the rays are laid over */
    int32_t num_samples;         /* rays per pixel, >= 1 (need not be a square) */
    int32_t integrator;          /* rtg_integrator */
    int32_t pt_flags;            /* rtg_pt_flags */
    int32_t pad[3];              /* must be 0 */
} rtg_ray_image;
int32_t rtg_render_rays(rtg_scene* scene, const rtg_ray_image* image, const rtg_ray* rays,
                        const rtg_render_opts* opts, float* rgb_out);
int32_t rtg_render_rays_device(rtg_scene* scene, const rtg_ray_image* image, const rtg_ray* rays_device,
                               const rtg_render_opts* opts, float* rgb_out_device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTG_H_ */
