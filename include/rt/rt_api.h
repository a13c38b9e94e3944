/* rt_api.h -- C ABI of the MI355X-native ray-traversal library (librtamd.so).
 *
 * Drop-in boundary for the reference's CPU render path (plindhorst/Ray-Tracing-Project):
 *   Flyscene::raytraceScene(int width, int height)      src/flyscene.hpp:65, src/flyscene.cpp:250-297
 *     -> traceRayThread (ray generation)                 src/flyscene.cpp:299-314
 *     -> traceRay / calculateMinimumFace / shadow / calculateColor   src/flyscene.cpp:317-614
 * The GL-free Flyscene mirror (ray-tracing-project_amd/host/flyscene.hpp) keeps initialize(w,h) and
 * raytraceScene(w,h) and calls rt_render() for the whole frame, then writes result.ppm with
 * rt_write_ppm() (= Tucano::ImageImporter::writePPMImage, tucano/utils/ppmIO.hpp:135-156).
 *
 * Conventions: plain C types only; every call returns 0 (RT_OK) or a negative rt_status; the message
 * of the last failure on the calling thread is rt_last_error(). No exceptions cross the ABI. A scene
 * handle is used from one host thread at a time. The caller owns every input array and output buffer;
 * the library copies the scene to the device at rt_scene_create(). There is no CPU fallback: every
 * render/trace entry point runs the gfx950 kernels and fails with RT_ERR_NO_DEVICE without a GPU.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API_VERSION 4  /* 4: multi-device scenes (rt_scene_opts.n_devices/devices, rt_synchronize_devices);
                             3: rt_stats.wave_node_bytes, RT_BUILDER_SBVH */

typedef enum rt_status {
  RT_OK = 0,
  RT_ERR_INVALID = -1,   /* bad argument / malformed input */
  RT_ERR_IO = -2,        /* file could not be opened / written */
  RT_ERR_NOMEM = -3,     /* host or device allocation failed */
  RT_ERR_HIP = -4,       /* HIP runtime error (message in rt_last_error) */
  RT_ERR_NO_DEVICE = -5, /* no GPU, or the scene was created host-only */
  RT_ERR_UNSUPPORTED = -6
} rt_status;

/* Tucano::Material::Mtl fields the ray tracer reads (tucano/materials/mtl.hpp:22-40) */
typedef struct rt_material {
  float ka[3], kd[3], ks[3];
  float shininess;        /* Ns */
  float optical_density;  /* Ni */
  float dissolve;         /* d  */
} rt_material;

/* ---------------------------------------------------------------------------------------------
 * Host-side scene ingest with Tucano semantics (no GPU needed)
 * ------------------------------------------------------------------------------------------- */
typedef struct rt_mesh rt_mesh;

/* Tucano::MeshImporter::loadObjFile (tucano/utils/objimporter.hpp:117-351) + Mesh::normalizeModelMatrix
 * (tucano/model.hpp:169-173), as Flyscene::initialize does (src/flyscene.cpp:18-22). */
int rt_mesh_load_obj(const char* path, rt_mesh** out);
/* Same ingest from memory: v3 [nv][3]; vn3 [nv][3] or NULL (then normals are computed as
 * computeNormals, objimporter.hpp:81-106); index groups as usemtl groups (group_index_counts are
 * index counts, multiples of 3); materials [n_materials]. */
int rt_mesh_from_arrays(int32_t n_vertices, const float* v3, const float* vn3, int32_t n_groups,
                        const int32_t* group_index_counts, const uint32_t* indices,
                        const int32_t* group_material, int32_t n_materials,
                        const rt_material* materials, rt_mesh** out);
void rt_mesh_destroy(rt_mesh* m);

/* Borrowed view of a prepared mesh, in the layout Flyscene holds after initialize(). */
typedef struct rt_mesh_desc {
  int32_t n_vertices;
  const float* vertices;            /* [n_vertices][4] object space, w = 1 (Mesh::vertices, mesh.hpp:292) */
  const float* vertex_normals;      /* [n_vertices][3] (Mesh::normals, mesh.hpp:293)              */
  int32_t n_faces;
  const uint32_t* face_vertex_ids;  /* [n_faces][3] (Face::vertex_ids, mesh.hpp:242)              */
  const float* face_normals;        /* [n_faces][3] (Face::normal, mesh.hpp:245; createFaces :475-477) */
  const int32_t* face_material_ids; /* [n_faces] (Face::material_id), -1 = none                   */
  int32_t n_materials;
  const rt_material* materials;     /* Flyscene::materials (flyscene.hpp:151)                     */
  float shape_model_matrix[16];     /* Mesh::getShapeModelMatrix(), column-major (model.hpp:102-105) */
} rt_mesh_desc;

int rt_mesh_get_desc(const rt_mesh* m, rt_mesh_desc* out);

/* Deterministic synthetic triangle soup used by the C3/C4 workloads: n_tris triangles, unshared
 * vertices v3_out [3*n_tris][3]; SplitMix64(seed); centres U[-0.5,0.5)^3, vertex jitter U[-0.01,0.01)^3. */
void rt_generate_soup(int32_t n_tris, uint64_t seed, float* v3_out);

/* Tucano::ImageImporter::writePPMImage (tucano/utils/ppmIO.hpp:135-156): P3, row 0 first,
 * min(255, (int)(255*c)). rgb is [H][W][3]. */
int rt_write_ppm(const char* path, const float* rgb, int32_t width, int32_t height);
/* The same P3 text from 8-bit values (rt_frame_download_rgb8); byte-identical to rt_write_ppm whenever
 * that download reported exact = 1. */
int rt_write_ppm_rgb8(const char* path, const uint8_t* rgb8, int32_t width, int32_t height);

/* ---------------------------------------------------------------------------------------------
 * Scene (device-resident acceleration structure)
 * ------------------------------------------------------------------------------------------- */
#define RT_DEVICE_NONE (-2) /* host-only scene: preparation + inspection, no upload, no rendering */

typedef struct rt_scene_opts {
  int32_t device;         /* HIP device ordinal; -1 = current device; RT_DEVICE_NONE = host only */
  int32_t min_faces;      /* Flyscene::MIN_FACES (flyscene.hpp:168), default 300 */
  int32_t max_boxes;      /* Flyscene::MAX_BOXES (flyscene.hpp:169), default INT32_MAX */
  int32_t leaf_size;      /* BVH leaf size bound (1..16), 0 = default (4 for SAH, 1 for the GPU LBVH) */
  rt_material default_material; /* Flyscene::ka/kd/ks/shininess defaults (flyscene.hpp:179-184) */
  float background[3];    /* Flyscene::BACKGROUND_COLOR (flyscene.hpp:175) */
  int32_t frames_in_flight; /* rt_render_async frames that may execute concurrently (1..4, default 4):
                             * each in-flight frame has its own stream and frame buffers; frames stay
                             * independent and rt_frame_download returns the most recent one. A frame
                             * alone on the GPU is dispatched longest-first from an earlier frame's wave
                             * costs (small scenes also split their costliest waves); results never
                             * depend on the dispatch order */
  int32_t builder;          /* the traversal tree's builder (results never depend on it):
                             * RT_BUILDER_SBVH_GPU (rt_scene_opts_default: SAH with spatial splits built on
                             * the device, 1M faces ~0.1 s of kernels; host RT_BUILDER_SBVH without a device or
                             * when the tree would be too deep), RT_BUILDER_SBVH (the same tree quality on the
                             * host; 1M faces 2-5 s), RT_BUILDER_SAH (host binned SAH without
                             * splits: ~4x faster build, ~5% slower traversal) or RT_BUILDER_LBVH_GPU
                             * (Morton/radix-sort/Karras build on the device in milliseconds;
                             * falls back to RT_BUILDER_SAH when the tree would be too deep) or
                             * RT_BUILDER_PLOC_GPU (parallel locally-ordered clustering on the
                             * device in milliseconds; same fallback) or RT_BUILDER_SAH_GPU (the host
                             * binned-SAH algorithm run top-down on the device, one level per round of
                             * launches; same fallback) or RT_BUILDER_SBVH_GPU (the same with the host
                             * SBVH's spatial splits; same fallback) */
  int32_t box_builder;      /* the reference box partition (generateBoundingBoxes): RT_BOXES_GPU (default since
                             * round 4; host-only scenes use the host builder) or RT_BOXES_HOST (parallel
                             * passes on the host); RT_BOXES_GPU (one launch per pass,
                             * one workgroup per box; identical boxes and face order; scenes with
                             * non-finite vertex coordinates use the host builder) */
  int32_t wide_tree;        /* 1: also build the fp32 4-wide tree (eight per-octant copies of 128-B nodes in
                             * HBM: ~8x the binary tree's node bytes) and walk it for PRIMARY packets whose
                             * rays share a direction octant. 0 (default): the binary tree only -- measured
                             * equal speed at a quarter of the memory. Results are
                             * identical either way (API 3) */
  /* Multi-device rendering in one process (API 4; SURVEY 8(b) b2 / 8(e) e1 -- the reference's frame
   * driver is one process, flyscene.cpp:266-289): n_devices > 1 renders every frame on the listed HIP
   * devices together. The scene is built once (on devices[0]) and replicated to every other listed
   * device by peer copy over xGMI; each frame's 16x16 tiles are split into 64x64-pixel super-tiles
   * interleaved over the devices (the rt_frame shard layout: device k of D renders shard
   * shard_index + shard_count * k of shard_count * D), each device renders on its own streams, and the
   * frame is assembled in the caller's buffer from each device's tiles (packed on the device, copied
   * through pinned host memory by a host worker per device): no collective. Entries may repeat (two
   * replicas sharing one GPU). n_devices 0 (default) or 1: one device, `device` (n_devices 1: devices[0]);
   * RT_DEVICES_ALL: every visible device. Results are bit-identical to a one-device render. Ray-list
   * queries (rt_trace_*), diagnostics and rt_frame_pack_shard_rgb8 use devices[0] only. */
  int32_t n_devices;
  int32_t devices[16];      /* RT_MAX_DEVICES */
} rt_scene_opts;

#define RT_MAX_DEVICES 16
#define RT_DEVICES_ALL (-1)

#define RT_BUILDER_SAH 0
#define RT_BUILDER_LBVH_GPU 1
#define RT_BUILDER_SBVH 2
#define RT_BUILDER_PLOC_GPU 3
#define RT_BUILDER_SAH_GPU 4
#define RT_BUILDER_SBVH_GPU 5
#define RT_BOXES_HOST 0
#define RT_BOXES_GPU 1

void rt_scene_opts_default(rt_scene_opts* o);

typedef struct rt_scene rt_scene;

/* Builds the reference's flat box partition (generateBoundingBoxes, flyscene.cpp:399-428, whose box
 * order defines closest-hit tie-breaking) and the traversal BVH, then uploads both. At most 2^25 - 1
 * faces (node and triangle records are addressed by 32-bit byte offsets); more: RT_ERR_INVALID. */
int rt_scene_create(const rt_mesh_desc* mesh, const rt_scene_opts* opts, rt_scene** out);
void rt_scene_destroy(rt_scene* s);

typedef struct rt_scene_info {
  int32_t n_faces, n_vertices, n_ref_boxes;
  int32_t bvh_nodes, bvh_leaves, bvh_depth;
  int64_t device_bytes;
  double build_ms;        /* host preparation (boxes + BVH) */
  int32_t device;         /* RT_DEVICE_NONE for host-only scenes */
  double prep_ms;         /* phases of rt_scene_create: per-vertex / per-face invariants, */
  double boxes_ms;        /* the reference box partition, */
  double bvh_ms;          /* the BVH build(s), */
  double upload_ms;       /* the device upload */
  int32_t builder;        /* the builder actually used (RT_BUILDER_*) */
  double bvh_gpu_ms;      /* device time of the LBVH kernels (RT_BUILDER_LBVH_GPU) */
  int32_t box_builder;    /* the box partition builder actually used (RT_BOXES_*) */
  double boxes_gpu_ms;    /* device time of the GPU box partition (RT_BOXES_GPU) */
  int32_t wide_nodes;     /* fp32 4-wide nodes per octant copy (0: no wide tree) (API 3) */
  int32_t wide_depth;     /* its depth */
  int32_t n_devices;      /* devices rendering the scene's frames (API 4; 1 for a single-device scene,
                             0 host-only); device_bytes sums over them */
  double replicate_ms;    /* time to replicate the device data to devices[1..] (0: one device) */
} rt_scene_info;

int rt_scene_get_info(const rt_scene* s, rt_scene_info* out);

/* Binary scene cache: rt_scene_save writes everything rt_scene_create derived from
 * the mesh (object and world vertices, unit normals, the reference box partition and its face order, the BVHs and
 * triangle records; versioned, with a content hash); rt_scene_load restores it and uploads it without
 * OBJ parsing or any build. The build parameters (min_faces, max_boxes, leaf_size) come from the file;
 * device, frames_in_flight, default_material and background from opts (NULL = defaults). A truncated,
 * corrupt or foreign file fails with RT_ERR_IO. Renders of a loaded scene equal the original's bit for
 * bit. */
int rt_scene_save(const rt_scene* s, const char* path);
int rt_scene_load(const char* path, const rt_scene_opts* opts, rt_scene** out);
/* reference boxes: bounds6 [n][6] (low xyz, high xyz, object space), counts [n], face_order [n_faces]
 * (faces in reference iteration order: box creation order, then in-box order). NULL = skip. */
int rt_scene_ref_boxes(const rt_scene* s, float* bounds6, int32_t* counts, int32_t* face_order);

/* ---------------------------------------------------------------------------------------------
 * Moving geometry: a scene's vertices updated in place (additive; RT_API_VERSION stays 4)
 *
 * rt_scene_update(s, mesh, stats) replaces the scene's geometry by `mesh`, which must have the scene's
 * topology: the same n_vertices, n_faces and n_materials, and face_vertex_ids and face_material_ids equal
 * element for element -- anything else returns RT_ERR_INVALID and leaves the scene exactly as it was. Everything
 * else is read again: vertices, vertex_normals, face_normals, shape_model_matrix and materials (a caller who
 * keeps the old model matrix writes it into the description; rt_mesh_from_arrays re-ingests moved vertices).
 *
 * Contract: after RT_OK every query -- rt_render*, rt_render_lit*, rt_render_views*, rt_render_ss in every
 * mode and depth, rt_trace_* and rt_trace_stream* under any flags, rt_scene_ref_boxes, rt_scene_ray_bounds,
 * rt_debug_ray, rt_debug_scene_flags' per-face flags -- gives, bit for bit, what it gives on a scene that
 * rt_scene_create makes from `mesh` with this scene's options. The per-face data (world vertices, normals,
 * plane distances, the reference boxes with their ranks, the flags, the static pad, the certificate range) is
 * derived again by rt_scene_create's own stages; the traversal tree keeps its topology and leaf order and has
 * its boxes refit, and since results never depend on the builder (rt_scene_opts.builder: the tree only
 * culls) any conservative tree gives the same bits. Only speed may differ: rt_debug_tree_cost tells when a
 * scene is better created anew.
 *
 * The call is synchronous: it first waits for the scene's frame-slot streams (as rt_synchronize does; the last
 * frame stays downloadable), for the latest list call (rt_trace_stream*, any flags) on every caller stream that
 * carried one, and for the latest view batch (batches on several streams run one after the other); on return the
 * device data is the new geometry. Light sets, frame slots, streams and scratch stay valid. Box colours stay
 * unless the number of reference boxes changed (then they are "not set yet" again).
 *
 * The tree is refit on the device (devices[0]; replicas receive the changed regions by device copy) unless the
 * scene is host-only or the new coordinates are not finite and below 1e30 in magnitude; then on the host.
 * Only the refusals (RT_ERR_INVALID, RT_ERR_UNSUPPORTED) leave the scene as it was. After any other error (a
 * device allocation or copy that failed) the host half already holds the new geometry and the device data may be
 * old or half-written: update the scene again, successfully, or destroy it before any further query.
 * Refused: scenes created with wide_tree = 1 return RT_ERR_UNSUPPORTED in this version (the fp32 4-wide
 * tree's eight octant copies share the node allocation and are not refit).
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_SCENE_UPDATE 1
typedef struct rt_update_stats {
  double prep_ms;           /* host: per-vertex / per-face invariants */
  double boxes_ms;          /* the reference-box partition (by the scene's box_builder) */
  double records_ms;        /* host: face records (ranks, boxes, flags), pad, certificate range */
  double upload_ms;         /* host-to-device copies (and the replicas' copies) */
  double refit_ms;          /* the refit: device events around the kernels, or the host refit's wall time */
  double total_ms;          /* the whole call after its waits */
  int32_t bounds_on_device; /* 1: the tree's boxes were refit on the device, 0: on the host */
  double sah_cost;          /* rt_debug_tree_cost(k_trav 0.7) out[0] after the update */
} rt_update_stats;
int rt_scene_update(rt_scene* s, const rt_mesh_desc* mesh, rt_update_stats* stats /* may be NULL */);
/* ---------------------------------------------------------------------------------------------
 * Device-resident geometry updates (additive; feature test: RT_HAS_DEVICE_UPDATE; RT_API_VERSION stays 4)
 *
 * rt_scene_update_device(s, g, hip_stream, stats) is rt_scene_update for a caller whose geometry lives in device
 * memory (a mesh deformed by kernels or torch every step): the three coordinate arrays are read where they are,
 * and every stage of the update -- the per-vertex and per-face invariants, the reference-box partition with its
 * ranks, the face flags, the static pad's bounds, the refit -- runs on the scene's device (devices[0]; replicas
 * receive the changed regions by device copy, as for rt_scene_update). The topology is the scene's own (counts,
 * face_vertex_ids, face_material_ids) and is not passed again. shape_model_matrix and materials are host
 * pointers; NULL keeps the scene's.
 *
 * Contract: after RT_OK the scene is, bit for bit, the scene rt_scene_update produces from a host rt_mesh_desc
 * holding the same three arrays, matrix and materials -- hence the scene rt_scene_create makes from them: every
 * query of the rt_scene_update contract, and rt_scene_ref_boxes, rt_scene_ray_bounds, rt_debug_scene_flags,
 * rt_debug_scene_records, rt_debug_validate_bvh, rt_debug_tree_cost, rt_scene_save, rt_debug_ray. The host half
 * of the scene is refreshed from the device at its first host reader; nothing is computed twice.
 *
 * hip_stream is the stream on which the caller produced the arrays: the library reads them behind an event it
 * records there (NULL: the default stream). The call is synchronous, with rt_scene_update's waits; on return the
 * device data is the new geometry and the caller's arrays are no longer read.
 *
 * Refusals, each checked before anything is queued and leaving the scene exactly as it was: a NULL scene or
 * geometry, a NULL array while its count is positive, a replica handle -> RT_ERR_INVALID; a wide_tree = 1 scene
 * -> RT_ERR_UNSUPPORTED; a host-only scene -> RT_ERR_NO_DEVICE; an array that is host memory or another
 * device's -> RT_ERR_INVALID. Any later failure has rt_scene_update's semantics: update again, successfully, or
 * destroy the scene.
 *
 * Coordinates that are NaN, infinite or beyond 1e30 in magnitude (object or world space) are detected on the
 * device; the call then downloads the three arrays and runs rt_scene_update on them (bounds_on_device = 0, the
 * stats rt_scene_update's). A scene without faces takes the same route. These are the only host fallbacks.
 *
 * rt_update_stats for this call: prep_ms = device time of the invariant kernels; boxes_ms = the partition (its
 * pass loop, on the device's timeline); records_ms = ranks, face flags and their small uploads; refit_ms = the
 * refit kernels; upload_ms = what follows on the host side: the box image, materials, a host-built scene's
 * quantised tree, the replicas' copies; total_ms = wall time after the waits.
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_DEVICE_UPDATE 1
typedef struct rt_device_geometry {
  const float* vertices;           /* device [n_vertices][4], object space (w as in rt_mesh_desc) */
  const float* vertex_normals;     /* device [n_vertices][3] */
  const float* face_normals;       /* device [n_faces][3]    */
  const float* shape_model_matrix; /* host [16] column-major, NULL = keep the scene's */
  const rt_material* materials;    /* host [n_materials of the scene], NULL = keep */
} rt_device_geometry;
int rt_scene_update_device(rt_scene* s, const rt_device_geometry* g, void* hip_stream,
                           rt_update_stats* stats /* may be NULL */);
/* The device-form image of the scene's records: which = 0 the binary nodes (64 B each), 1 the triangle records
 * in leaf order (64 B), 2 the per-slot shading records (48 B). Downloaded from the device for a device scene;
 * for a host-only scene built the way the upload builds it. *n_bytes = the image's size; out may be NULL
 * (size query), else capacity_bytes must hold it. */
int rt_debug_scene_records(rt_scene* s, int32_t which, int64_t capacity_bytes, void* out, int64_t* n_bytes);

/* ---------------------------------------------------------------------------------------------
 * Camera, lights, frames
 * ------------------------------------------------------------------------------------------- */
typedef struct rt_camera {
  float view_matrix[16]; /* Camera::view_matrix (Affine3f), column-major (tucano/camera.hpp) */
  float viewport[4];     /* Camera::viewport: x, y, width, height */
  float fovy;            /* degrees */
  float aspect_ratio;
} rt_camera;

/* Flycamera default pose (eye (0,0,2), tucano/utils/flycamera.hpp:76-86) after translate(dx,dy,dz)
 * and updateViewMatrix(), with Flyscene::initialize's projection (fovy 60, aspect W/H, viewport). */
void rt_camera_flycam(int32_t width, int32_t height, float dx, float dy, float dz, rt_camera* out);

typedef struct rt_light {
  float position[3]; /* point: Flyscene::lights[i].first (flyscene.hpp:132); directional: the vector the
                        reference stores as get<0>(dirLights[i]) (flyscene.hpp:135) and uses as the light
                        direction as is (calculateColor, flyscene.cpp:610-612) */
  float color[3];    /* Flyscene::lights[i].second / get<1>(dirLights[i]) */
  int32_t kind;      /* RT_LIGHT_POINT or RT_LIGHT_DIRECTIONAL */
} rt_light;

#define RT_LIGHT_POINT 0
#define RT_LIGHT_DIRECTIONAL 1
/* calculateColor sums every point light (in order), then every directional light (in order); the
 * library applies that order whatever the order of the array. */
#define RT_MAX_LIGHTS 32

/* Light helpers. The reference draws sphere jitter from the C library's rand()
 * without seeding it (flyscene.cpp:529-538); rt_rand_state reproduces glibc's rand() (TYPE_3 additive
 * feedback generator, RAND_MAX 2^31-1), so seed 1 gives the sequence of a fresh reference process. */
typedef struct rt_rand_state {
  uint32_t r[34];
  uint32_t k;
} rt_rand_state;
void rt_rand_seed(rt_rand_state* st, uint32_t seed);
int32_t rt_rand(rt_rand_state* st);
/* Flyscene::sphericalLight + addLight('s') (flyscene.cpp:212-239, 529-538): n_points jittered point lights
 * (offset (-r + rand()/(RAND_MAX/(2r))) per axis, x then y then z) each with colour/(n_points+1), then the
 * centre light with colour/(n_points+1); writes n_points + 1 lights to out and returns that count. */
int32_t rt_lights_spherical(const rt_light* centre, float radius, int32_t n_points, rt_rand_state* rng, rt_light* out);
/* addLight('d') (flyscene.cpp:242-246): the "direction" the reference stores is screenToWorld(viewport
 * centre), a point (a point used as a direction); kind = RT_LIGHT_DIRECTIONAL. */
void rt_light_directional(const rt_camera* cam, const float color[3], rt_light* out);

enum { RT_MODE_PRIMARY = 0, RT_MODE_FULL = 1, RT_MODE_BOX_COLORS = 2 };

typedef struct rt_frame {
  int32_t width, height;
  int32_t mode;        /* RT_MODE_PRIMARY: closest hit + unshadowed Phong (traceRay at depth limit 1);
                          RT_MODE_FULL: reference traceRay as-is (shadow per light + 1 reflection);
                          RT_MODE_BOX_COLORS: traceRay with RENDER_BOUNDINGBOX_COLORED_TRIANGLES set
                          (flyscene.hpp:166, flyscene.cpp:334-348): a hit pixel is the sum of the colours
                          of every reference box that hasFace() the closest face, unclamped, no shading,
                          shadows or reflection (a miss: the background); colours: rt_scene_set_box_colors */
  int32_t shard_index; /* this device renders its share of the frame's 16x16-pixel tiles: with
                          shard_count > 1 the tiles are grouped into 4x4-tile super-tiles (64x64 pixels;
                          row-major over the frame, partial at the right / bottom edges) and super-tile s
                          belongs to shard s % shard_count (an XCD's concurrent waves then trace
                          neighbouring pixels); rt_frame_shard_tiles lists them */
  int32_t shard_count; /* 1 = whole frame */
  int32_t flags;       /* RT_FRAME_* */
  int32_t max_depth;   /* traceRay's recursion limit (Flyscene::max_depth, flyscene.hpp:142; the reference
                          fixes 2): 0 = the mode's own (PRIMARY 1, FULL 2); 1..RT_MAX_TRACE_DEPTH = trace
                          that many levels (primary hit + max_depth-1 reflection bounces), with shadow rays
                          in FULL mode and without in PRIMARY mode. The FULL/2 and PRIMARY/1 cases run the
                          tuned kernels; other depths one generic kernel (same arithmetic, same bits).
                          RT_MODE_BOX_COLORS returns before any reflection, so every depth >= 1 renders
                          the same frame there (0 and 1..16 accepted, one kernel). */
} rt_frame;

#define RT_MAX_TRACE_DEPTH 16

#define RT_FRAME_WRITE_HITS 1 /* also record per-pixel face index and t (rt_frame_download) */
#define RT_FRAME_STATS 2      /* counting run: per-ray node visits / triangle tests (slower) */
#define RT_FRAME_TIMELINE 4   /* diagnostics: each wave of the render kernel records its start / end clocks
                                 and the CU it ran on (rt_debug_timeline); PRIMARY and FULL kernels */
#define RT_FRAME_WAVE_STATS 8 /* diagnostics, with RT_FRAME_STATS: each wave of the counting run also records its own
                                 counts (rt_debug_wave_stats). Only at the mode's own recursion limit (max_depth 0,
                                 or 1 for PRIMARY / 2 for FULL): with any other max_depth the frame is refused
                                 with RT_ERR_UNSUPPORTED, the generic-depth kernel keeps no per-wave counts */

typedef struct rt_stats {
  double kernel_ms;         /* device time of the render kernels since the previous rt_synchronize,
                               summed over launches (HIP events on the scene's stream) */
  int64_t launches;         /* render launches covered by kernel_ms */
  double trace_kernel_ms;   /* part of kernel_ms spent in the traversal kernel (PRIMARY: first of the
                               two kernels of a frame; FULL: the whole single kernel) */
  int64_t primary_rays;     /* pixels traced by this call */
  int64_t total_rays;       /* primary + shadow + reflection rays issued */
  int64_t hits;             /* primary rays that hit */
  int64_t node_visits;      /* RT_FRAME_STATS: sum over rays of interior nodes whose box the ray hit */
  int64_t tri_tests;        /* RT_FRAME_STATS: sum over rays of triangle tests */
  int64_t wave_node_fetches;/* RT_FRAME_STATS: node records fetched (once per wave) */
  int64_t wave_tri_fetches; /* RT_FRAME_STATS: triangle records fetched (once per wave) */
  int64_t wave_node_bytes;  /* RT_FRAME_STATS: bytes of the node records fetched (64 per binary record,
                               128 per fp32 4-wide record; API 3) */
} rt_stats;

/* Renders the frame (this shard's tiles) on the scene's device and copies it into out_rgb
 * ([H][W][3], row 0 = top, untouched outside this shard). Synchronous. */
int rt_render(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights,
              const rt_frame* frame, float* out_rgb, rt_stats* stats);

/* Device-resident variant for benchmarking: renders into the scene's device frame buffer and returns
 * without synchronising; rt_synchronize() waits and fills the stats of the last render. */
int rt_render_async(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights,
                    const rt_frame* frame);
int rt_synchronize(rt_scene* s, rt_stats* stats);
/* rt_synchronize with the figures of every device of a multi-device scene (API 4): per_device[k] (k <
 * capacity, may be NULL) = device k's own stats (its kernel_ms, primary_rays, ...). In *stats (may be
 * NULL) ray counts and counters are summed over the devices and kernel_ms / trace_kernel_ms are the
 * maximum over the devices (the frames' critical path); launches are per device. Returns the number of
 * devices (>= 1) or a negative rt_status. rt_synchronize(s, st) == rt_synchronize_devices(s, st, 0, NULL). */
int rt_synchronize_devices(rt_scene* s, rt_stats* stats, int32_t capacity, rt_stats* per_device);
/* copies the last frame from the device: rgb [H][W][3]; face [H][W] (-1 miss) and t [H][W] need
 * RT_FRAME_WRITE_HITS. NULL = skip. capacity_pixels: the pixels each given buffer holds; smaller than
 * the last frame's W x H -> RT_ERR_INVALID, nothing written. */
int rt_frame_download(rt_scene* s, int64_t capacity_pixels, float* rgb, int32_t* face, float* t);
/* Output path: the last frame converted on the device to writePPMImage's 8-bit
 * values min(255, (int)(255*c)) and downloaded at 3 B/px. *exact (may be NULL) = 1 when every value
 * was in 0..255, i.e. the bytes are exactly the PPM's numbers; 0 when some colour was NaN or negative
 * (clamped to 0 here; rt_frame_download + rt_write_ppm reproduce the reference's text then).
 * capacity_pixels: pixels the buffer holds (3 bytes each), checked as in rt_frame_download. */
int rt_frame_download_rgb8(rt_scene* s, int64_t capacity_pixels, uint8_t* rgb8, int32_t* exact);

/* Multi-GPU frame assembly (f3). Each rank's slice holds the 8-bit values of its own 16x16 tiles
 * (rt_frame.shard_index/shard_count of its last frame) in shard tile order, rt_frame_shard_bytes() long
 * (equal for all ranks, so one RCCL gather / all-gather of the slices brings the frame to one GPU);
 * rt_frame_unpack_shards_rgb8 turns the concatenated slices into the H x W x 3 frame. Both pointers are
 * device memory on the scene's / the given device (e.g. torch tensors' data_ptr()); both calls return
 * after their device work is complete, and the caller orders any earlier writes to those buffers made on
 * other streams (the library's streams do not synchronise with the legacy default stream). */
int64_t rt_frame_shard_bytes(int32_t width, int32_t height, int32_t shard_count);
/* The 16x16 tiles shard shard_index of shard_count renders, in its slot order (the order of its packed
 * slice; slots of super-tile tiles outside the frame are skipped here and zero in the slice): writes the
 * first min(n, capacity) as tiles_xy [..][2] = (tile x, tile y) (NULL = count only) and returns n, the
 * shard's tile count (0 for invalid arguments). */
int32_t rt_frame_shard_tiles(int32_t width, int32_t height, int32_t shard_index, int32_t shard_count, int32_t* tiles_xy,
                             int32_t capacity);
int rt_frame_pack_shard_rgb8(rt_scene* s, void* dst_device);
int rt_frame_unpack_shards_rgb8(const void* packed_device, int32_t shard_count, int32_t width, int32_t height,
                                void* frame_device, int32_t device);

/* Box colours of RT_MODE_BOX_COLORS. The reference draws them in generateBoundingBoxes when its
 * RENDER_BOUNDINGBOX_COLORED_TRIANGLES flag is set (flyscene.cpp:422-427): BoundingBox::setRandomColor
 * per box in creation order, colour = Vector3f(rand() / (float)RAND_MAX, x3) (BoundingBox.cpp:163-165).
 * rt_box_colors_random reproduces that sequence from rng (NULL = seed 1: a fresh reference process,
 * whose first rand() calls these are) into out3 [n_boxes][3], with the constructor's arguments
 * evaluated right to left as the reference's g++ (and x86-64 MSVC) build does: each box's first
 * rand() call is its blue channel, the third its red (C++ leaves the order unspecified; pinned by
 * tests/golden/boxcolor_kat.bin from that expression compiled here). Callers of another compiler's
 * order pass their own colours to rt_scene_set_box_colors. rt_scene_set_box_colors gives the scene
 * its colours ([n_ref_boxes][3]; NULL = rt_box_colors_random(n_ref_boxes, NULL)); a scene that renders
 * RT_MODE_BOX_COLORS without them gets the NULL colours. The per-face sums are computed on the device
 * at the first box-colour frame after the colours change (one pass over faces x boxes). */
int rt_box_colors_random(int32_t n_boxes, rt_rand_state* rng, float* out3);
int rt_scene_set_box_colors(rt_scene* s, const float* colors3);

/* calculateMinimumFace (flyscene.cpp:373-396) for n rays on the device: face -1 = miss (t = +inf) */
int rt_trace_closest(rt_scene* s, int32_t n, const float* origins3, const float* dirs3, int32_t* face,
                     float* t, float* P3);
/* shadow(P, L) (flyscene.cpp:510-526) for n rays on the device: blocked 1/0 */
int rt_trace_shadow(rt_scene* s, int32_t n, const float* P3, const float* L3, int32_t* blocked);
/* calculateMinimumFace plus interpolateNormal at the hit (N [n][3], zero on a miss) */
int rt_trace_closest_normal(rt_scene* s, int32_t n, const float* o3, const float* d3, int32_t* face, float* t,
                            float* P3, float* N3);
/* traceRay(o, d, 0) (flyscene.cpp:317-371, max_depth 2 with shadows: the FULL frame's colour path) for
 * arbitrary rays: colour rgb [n][3], first-hit face (-1 miss) and t (NULL = skip). */
int rt_trace_color(rt_scene* s, int32_t n, const float* o3, const float* d3, const rt_light* lights, int32_t n_lights,
                   float* rgb3, int32_t* face, float* t);

/* ---------------------------------------------------------------------------------------------
 * Ray streams: the same three queries on ray lists that already live in device memory, enqueued on the
 * caller's stream (feature test: RT_HAS_RAY_STREAMS; the API version stays 4).
 *
 * rt_trace_stream(s, query, flags, rays, lights, n_lights, hip_stream)
 *   query       RT_RAYS_CLOSEST = rt_trace_closest_normal, RT_RAYS_SHADOW = rt_trace_shadow, RT_RAYS_COLOR =
 *               rt_trace_color; the values written are exactly the host-pointer call's (a miss: face -1,
 *               t +inf, P and N zero). Nothing is written at index n or beyond.
 *   rays        every pointer is device (or managed) memory of the scene's device -- devices[0] of a
 *               multi-device scene -- e.g. a torch tensor's data_ptr(). a3 / b3 are read, the outputs the
 *               query names are written: CLOSEST face and t (required), P3 and N3 (optional); SHADOW blocked
 *               (required); COLOR rgb3 (required), face and t (optional). lights / n_lights: COLOR only,
 *               host memory, as rt_trace_color.
 *   hip_stream  non-NULL: the caller's hipStream_t (torch: torch.cuda.current_stream().cuda_stream). All work
 *               is enqueued there in order and the call returns without waiting; nothing in it synchronises
 *               the device except a growth of the reorder scratch. NULL: the scene's own stream, and the call
 *               returns after completion, as the host-pointer calls do.
 *   flags       RT_RAYS_REORDER: trace the rays in coherence order instead of list order. Each ray gets a
 *               32-bit key on the device (its origin's cell in the scene's bounds, its direction's octant
 *               and cell; csrc/rt_raykey.h), the (key, index) pairs are radix-sorted, and packet lanes take
 *               their rays through that permutation, writing each result at its ray's own index. A ray's
 *               result never depends on the rays sharing its wave, so every output bit equals the in-order
 *               call's; what changes is how many node records the waves fetch. Opt-in: the key and sort
 *               cost time that only an unordered list pays back (README.md has the measured figures).
 *               Lists of at most 64 rays are one packet and are traced as given. The scratch (16 B per ray
 *               plus the sort's temporary storage, about 32 B per ray together) belongs to the scene, grows
 *               geometrically -- the one place a call may hipMalloc / hipFree and so stall -- and is freed
 *               with the scene. Calls on different streams are ordered on it by an event: the later stream
 *               waits for the earlier call's use. One host thread per scene, as everywhere.
 *               RT_RAYS_STATS: a counting run (slower): clears the scene's counters, then counts node visits,
 *               triangle tests and the per-wave node / triangle record fetches (rt_debug_counters slots
 *               0..3; 4 rays, 5 hits). Not available with the 4-wide A/B variant (RT_ERR_UNSUPPORTED).
 *   Checked before anything is enqueued: query and flags, n >= 0, the query's required outputs (n > 0), the
 *   lights, and every non-NULL pointer's memory (hipPointerGetAttributes: host memory or another device's
 *   returns RT_ERR_INVALID). n == 0 returns RT_OK and launches nothing. A host-only scene or a machine
 *   without a GPU returns RT_ERR_NO_DEVICE.
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_RAY_STREAMS 1
enum { RT_RAYS_CLOSEST = 0, RT_RAYS_SHADOW = 1, RT_RAYS_COLOR = 2 };
#define RT_RAYS_REORDER 1   /* trace in coherence order (results identical; needs scratch ~32 B/ray) */
#define RT_RAYS_STATS   2   /* counting run (slower): fills the scene's counters, read with rt_debug_counters */

typedef struct rt_ray_stream {      /* every pointer: device memory on the scene's device (devices[0]) */
  int32_t n;
  const float* a3;                  /* CLOSEST/COLOR: origins [n][3];  SHADOW: P [n][3] */
  const float* b3;                  /* CLOSEST/COLOR: directions;      SHADOW: L */
  int32_t* face; float* t;          /* CLOSEST (both required), COLOR (optional) */
  float* P3; float* N3;             /* CLOSEST, optional */
  int32_t* blocked;                 /* SHADOW, required */
  float* rgb3;                      /* COLOR, required */
} rt_ray_stream;

int rt_trace_stream(rt_scene* s, int32_t query, int32_t flags, const rt_ray_stream* rays,
                    const rt_light* lights, int32_t n_lights, void* hip_stream);
/* The primary rays of a width x height frame of cam as a device ray list: pixel (px, py) at index
 * py * width + px, exactly the origin and direction the frame kernels trace for it (traceRayThread,
 * flyscene.cpp:301-308). Both outputs [width * height][3], device memory, checked and enqueued as above. */
int rt_rays_camera(rt_scene* s, const rt_camera* cam, int32_t width, int32_t height,
                   float* origins3_device, float* dirs3_device, void* hip_stream);
/* The grid of the coherence keys: the world bounds of the scene's vertices (lo xyz, hi xyz). Host data. */
int rt_scene_ray_bounds(rt_scene* s, float bounds6[6]);
/* The keys RT_RAYS_REORDER gives n rays on a grid of bounds6, computed on the host by the function the device
 * runs (tests and diagnostics). Bit 31: a NaN / infinite component or an all-zero direction (sorted last). */
int rt_debug_ray_keys(int32_t query, int32_t n, const float* a3, const float* b3,
                      const float bounds6[6], uint32_t* keys_out);           /* host only, no device */
/* The order of the scene's last RT_RAYS_REORDER call: perm_out[k] = the index of the ray traced k-th (the
 * identity for a list of at most 64 rays); *n_out = that call's n. capacity smaller than n: RT_ERR_INVALID.
 * Waits for that call. */
int rt_debug_ray_order(rt_scene* s, int64_t capacity, uint32_t* perm_out, int64_t* n_out); /* last REORDER call */

/* ---------------------------------------------------------------------------------------------
 * traceRay for a device ray list at any recursion limit and in either mode: what rt_frame.mode / max_depth
 * are to frames (feature test: RT_HAS_RAY_DEPTH; the API version stays 4).
 *
 * rt_trace_stream_color(s, flags, rays, lights, n_lights, mode, max_depth, hip_stream)
 *   rays        a3 origins, b3 directions; rgb3 required, face and t optional (the first hit; a miss: -1, +inf).
 *               The other members are ignored.
 *   mode        RT_MODE_PRIMARY: no shadow rays; RT_MODE_FULL: a shadow ray per light per hit. Anything else:
 *               RT_ERR_INVALID ("bad mode").
 *   max_depth   0 = the mode's own limit (PRIMARY 1, FULL 2); 1..RT_MAX_TRACE_DEPTH; else RT_ERR_INVALID.
 *   Ray i's colour, face and t are exactly what rt_render writes for a pixel whose camera ray is ray i, in that
 *   mode at that depth: a primary miss gives the scene's background, the material state stays with the chain
 *   from level to level and the final ks folds the levels, as in the frame kernel (csrc/rt_trace_ray.h
 *   k_render_depth; the list kernel k_rays_depth runs a copy of its level loop).
 *   flags       RT_RAYS_REORDER, RT_RAYS_STATS as rt_trace_stream (the reorder groups level 0's rays).
 *               RT_RAYS_WAVEFRONT: trace level by level instead of chain by chain. Every level is a closest-hit
 *               stage over the rays still alive, a regroup of the hits, a shade stage over them (its shadow
 *               packets are then made of neighbouring hit points; PRIMARY mode and calls without lights have no
 *               shadow rays and shade inside the closest stage), and a regroup of the reflection rays for the
 *               next level; a last pass folds the levels and writes each ray's outputs at its own index. Without
 *               RT_RAYS_REORDER a regroup is a stable compaction (survivors keep list order), with it a stable
 *               sort by the coherence key of the stage's own rays (closest: origin and direction; shade: hit
 *               point and direction to the first light). Every output bit equals the flagless call's. No count
 *               is read back: each stage is launched for n and its packets leave early. Scratch: 124 + 12 D
 *               bytes per ray at depth D (172 B at 4, 316 B at 16; csrc/rt_wavefront.h) plus the sorts'
 *               temporary storage, scene-owned, grown geometrically and ordered across streams as the reorder
 *               scratch is; a failed allocation returns RT_ERR_NOMEM. Opt-in: README.md has what was measured.
 *               RT_RAYS_STATS with it: slots 4 (rays), 5 (primary hits), 6 (all rays) equal the in-order
 *               call's; slots 0..3 depend on the grouping.
 *   FULL at depth 0 or 2 without RT_RAYS_WAVEFRONT is rt_trace_stream(RT_RAYS_COLOR), same kernel. Every other
 *   combination runs binary-tree kernels only and returns RT_ERR_UNSUPPORTED under the 4-wide A/B variant.
 *   Checks, n == 0, host-only scenes and stream semantics: as rt_trace_stream. rt_trace_stream itself keeps
 *   refusing flag 4.
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_RAY_DEPTH 1
#define RT_RAYS_WAVEFRONT 4   /* rt_trace_stream_color only */
int rt_trace_stream_color(rt_scene* s, int32_t flags, const rt_ray_stream* rays,
                          const rt_light* lights, int32_t n_lights,
                          int32_t mode, int32_t max_depth, void* hip_stream);
/* The levels of the scene's last RT_RAYS_WAVEFRONT call (waits for it): *n_levels = its depth D; for d < D,
 * out2[2 d] = rays that entered level d's closest-hit stage, out2[2 d + 1] = how many of them hit. capacity
 * (levels) smaller than D, or no such call yet: RT_ERR_INVALID. out2 NULL: only *n_levels. */
int rt_debug_ray_levels(rt_scene* s, int32_t capacity, int64_t* out2, int32_t* n_levels);
/* After an RT_RAYS_WAVEFRONT | RT_RAYS_REORDER call rt_debug_ray_order returns level 0's order, the permutation
 * the plain RT_RAYS_REORDER call computes for that list; a wavefront call without the reorder leaves it alone. */

/* ---------------------------------------------------------------------------------------------
 * Light sets: frames and ray lists lit by any number of lights (feature test: RT_HAS_LIGHT_SETS; the API
 * version stays 4). Flyscene::lights / dirLights are unbounded vectors (flyscene.hpp:132-135; sphericalLight,
 * flyscene.cpp:529-538, adds nLightpoints + 1 of them at a time) and calculateColor loops over all of them
 * (:603-614). rt_render and its siblings carry at most RT_MAX_LIGHTS lights in the kernel arguments and keep
 * that cap; a light set holds up to RT_MAX_LIGHT_SET lights in device memory.
 *
 * rt_light_set_create(s, lights, n_lights, out)
 *   Copies n_lights lights from host memory in the order calculateColor applies them -- every point light in
 *   array order, then every directional light in array order; kind: anything that is not RT_LIGHT_DIRECTIONAL
 *   is a point light -- and uploads one copy to each device of the scene (devices[0..] of a multi-device
 *   scene). The set is immutable and belongs to s, so frames in flight cannot race with it. n_lights == 0 is a
 *   valid, empty set. n_lights < 0 or > RT_MAX_LIGHT_SET, n_lights > 0 with lights NULL, a NULL scene or out:
 *   RT_ERR_INVALID. On a host-only scene (RT_DEVICE_NONE) the set holds the host copy only: create, get and
 *   destroy work, rendering with it returns RT_ERR_NO_DEVICE.
 * rt_light_set_get(ls, capacity, out, n_out)
 *   The set's lights in the set's order; *n_out (may be NULL) = their number. out NULL: the count only.
 *   capacity smaller than the count: RT_ERR_INVALID, nothing written.
 * rt_light_set_destroy(ls)
 *   Waits for the scene's own streams (every device's frame slots), then frees the set. Sets still alive when
 *   their scene is destroyed are freed by rt_scene_destroy; such a handle must not be used afterwards. A set
 *   used by work enqueued on a caller's stream (rt_trace_stream_lit with hip_stream) must outlive that work:
 *   the library cannot wait for a stream it does not own, exactly as for the rt_ray_stream buffers.
 *
 * rt_render_lit / rt_render_lit_async: rt_render / rt_render_async with the set in place of lights, n_lights.
 *   Every mode, max_depth, shard, flag, rt_synchronize, the downloads and multi-device scenes behave as for
 *   rt_render; a pixel's colour, face and t are traceRay's with Flyscene::lights and dirLights equal to the set
 *   (RT_MODE_BOX_COLORS ignores lights). A set of another scene: RT_ERR_INVALID.
 *   A set of at most RT_MAX_LIGHTS lights is copied into the kernel arguments and takes exactly rt_render's
 *   path. A larger set is read from device memory by the generic traceRay kernel (k_render_depth; scalar loads
 *   indexed by the wave-uniform light number, the same arithmetic in the same order, hence the same bits as
 *   the kernel-argument path for the same lights), for PRIMARY and FULL at every depth; that kernel keeps no
 *   per-wave counts, so RT_FRAME_WAVE_STATS is refused there (RT_ERR_UNSUPPORTED).
 * rt_trace_stream_lit: rt_trace_stream_color with the set: the same flags (RT_RAYS_REORDER | RT_RAYS_STATS |
 *   RT_RAYS_WAVEFRONT), checks, stream semantics and handling of n == 0 and host-only scenes. Ray i gets exactly
 *   the values rt_render_lit writes for a pixel with that camera ray. Under RT_RAYS_WAVEFRONT | RT_RAYS_REORDER
 *   the shade stage's key uses the set's first light. Lists read the copy on the scene's device (devices[0]).
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_LIGHT_SETS 1
#define RT_MAX_LIGHT_SET 65536
typedef struct rt_light_set rt_light_set;

int rt_light_set_create(rt_scene* s, const rt_light* lights, int32_t n_lights, rt_light_set** out);
void rt_light_set_destroy(rt_light_set* ls);
int rt_light_set_get(const rt_light_set* ls, int32_t capacity, rt_light* out, int32_t* n_out);

int rt_render_lit(rt_scene* s, const rt_camera* cam, const rt_light_set* ls, const rt_frame* frame, float* out_rgb,
                  rt_stats* stats);
int rt_render_lit_async(rt_scene* s, const rt_camera* cam, const rt_light_set* ls, const rt_frame* frame);

int rt_trace_stream_lit(rt_scene* s, int32_t flags, const rt_ray_stream* rays, const rt_light_set* ls,
                        int32_t mode, int32_t max_depth, void* hip_stream);

/* ---------------------------------------------------------------------------------------------
 * View batches: many cameras of one scene rendered by one launch into device memory, on the caller's stream
 * (feature test: RT_HAS_VIEW_BATCHES; the API version stays 4). For many small views consumed on the GPU -- a
 * camera path, multi-view data, one camera per environment -- where a loop of rt_render_async is bound by its
 * per-frame host cost and rt_frame_download by the trip to host memory.
 *
 * rt_render_views(s, views, lights, n_lights, frame, hip_stream)
 *   Renders views->n_views cameras at frame->width x frame->height with the same lights, mode and max_depth. View
 *   v, pixel (px, py) -- row 0 = top -- gets exactly the colour, face and t that rt_render writes for
 *   cameras[v] with RT_FRAME_WRITE_HITS and rt_frame_download returns at (px, py): rgb[((v H + py) W + px) 3 ..],
 *   face / t[(v H + py) W + px]. Each camera carries its own view matrix, viewport, fovy and aspect ratio.
 *   cameras is host memory and is read before the call returns; rgb (required), face and t (each optional,
 *   independent of the other) are device memory of the scene's device. Nothing is written beyond
 *   n_views * H * W elements.
 *   frame: mode RT_MODE_PRIMARY or RT_MODE_FULL (RT_MODE_BOX_COLORS: RT_ERR_UNSUPPORTED); max_depth 0 (the
 *   mode's own) or 1..RT_MAX_TRACE_DEPTH; shard_count 0 or 1 with shard_index 0 (a sharded batch:
 *   RT_ERR_UNSUPPORTED); flags 0 or RT_FRAME_WRITE_HITS, which is ignored -- the face and t pointers say what is
 *   written (RT_FRAME_STATS, RT_FRAME_TIMELINE, RT_FRAME_WAVE_STATS: RT_ERR_UNSUPPORTED).
 *   hip_stream as in rt_trace_stream: non-NULL = everything is enqueued there in order and the call returns
 *   without waiting for the render; NULL = the scene's own stream, and the call returns after completion.
 *   Checks, before anything is enqueued: a NULL scene RT_ERR_INVALID; then a host-only scene or no GPU
 *   RT_ERR_NO_DEVICE; n_views outside 0..RT_MAX_VIEWS, more than RT_MAX_LIGHTS lights, NULL cameras or rgb with
 *   n_views > 0, an output pointer that is host memory or another device's: RT_ERR_INVALID; a batch of 2^26 or
 *   more 8x8-pixel blocks (n_views * 4 * ceil(W / 16) * ceil(H / 16); the launch's limit of 2^32 work-items,
 *   hence also below 2^31 blocks): RT_ERR_INVALID. n_views == 0 returns RT_OK and launches nothing.
 *   The camera records (the derived camera rt_render computes per frame) are uploaded through pinned memory into
 *   an array the scene owns, ordered across calls by events: a call may wait on the host for the previous call's
 *   camera upload, never for a render. The array is reused, so a batch on another stream than the previous
 *   batch's starts on the device after that batch's kernel: two batches on two streams are both correct but
 *   run one after the other. Batches on one stream are ordered by the stream. A batch never waits for frames
 *   of rt_render_async, and they never wait for it.
 *   A multi-device scene renders the batch on devices[0] alone, as the ray lists.
 * rt_render_views_lit: the same with a light set (rt_render_lit's result per view). A set of another scene:
 *   RT_ERR_INVALID. The set must outlive work enqueued on a caller's stream.
 * Kernels: PRIMARY at depth 1 runs k_views_primary (k_primary_fused's traversal and shading), everything else
 *   k_views_depth (k_render_depth's level loop; light sets in device memory selected as for frames). Blocks are
 *   dispatched in plain order: no cost map, no wave split, no timeline -- rt_render keeps those, and stays the
 *   better call for one large frame.
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_VIEW_BATCHES 1
#define RT_MAX_VIEWS 65536
typedef struct rt_view_batch {
  int32_t n_views;
  const rt_camera* cameras;  /* host memory [n_views]; may be freed or overwritten as soon as the call returns */
  float*   rgb;              /* device [n_views][H][W][3], row 0 = top; required when n_views > 0 */
  int32_t* face;             /* device [n_views][H][W], -1 = miss; optional */
  float*   t;                /* device [n_views][H][W], +inf = miss; optional, independent of face */
} rt_view_batch;

int rt_render_views(rt_scene* s, const rt_view_batch* views, const rt_light* lights, int32_t n_lights,
                    const rt_frame* frame, void* hip_stream);
int rt_render_views_lit(rt_scene* s, const rt_view_batch* views, const rt_light_set* ls,
                        const rt_frame* frame, void* hip_stream);
/* The plan of a batch (host only, no device; csrc/rt_dispatch.h plan_views, which rt_render_views reads for its
 * kernel and every refusal).
 * in[0..8] (n_in = 9): mode, max_depth, flags, shard_count, tiles_x, tiles_y (16x16-pixel tiles of one view),
 * n_views, kernel variant, the number of lights read from a light set in device memory (0 = none).
 * out[0..6] (n_out = 7): 0 kernel (0 none: an empty or refused batch, 1 k_views_primary, 2 k_views_depth),
 * 1 recursion limit, 2 units per view (one-wave blocks: 4 tiles_x tiles_y), 3 total blocks, 4 light source
 * (0 kernel arguments, 1 device memory, 2 device memory with the occluder cache), 5 whether the batch is refused,
 * 6 the status rt_render_views returns for it (RT_OK when not refused).
 * Variant bits read: 65536 (k_views_depth also at PRIMARY depth 1), 2097152 (k_views_primary on the binary tree),
 * 16777216 (no occluder cache); every other bit is ignored. */
int rt_debug_view_plan(const int64_t in[], int32_t n_in, int64_t out[], int32_t n_out);

/* ---------------------------------------------------------------------------------------------
 * Supersampled views: several rays per pixel, averaged in the launch (feature test: RT_HAS_SUPERSAMPLING; the API
 * version stays 4). A sample pattern is S offsets (ox_k, oy_k), 1 <= S <= RT_MAX_SAMPLES, each within [-1, 1].
 *
 * Sample k of pixel (px, py) of view v is exactly the pixel rt_render writes at (px, py) for cameras[v] with
 * viewport[0] replaced by viewport[0] - ox_k and viewport[1] by viewport[1] - oy_k, both float subtractions
 * (everything else of the camera unchanged): for a viewport origin of (0, 0), the reference's screenToWorld at the
 * float position (px + ox_k, py + oy_k). The pixel's colour is, per channel, ((c_0 + c_1) + ...) + c_{S-1} in that
 * order as float additions, divided by (float)S (correctly rounded); each c_k is traceRay's clamped colour (the
 * background on a primary miss). face and t are sample 0's. One sample at offset (0, 0) writes rt_render_views' bits.
 *
 * rt_sample_pattern_grid(nx, ny, out): the centres of an nx x ny grid of cells over the pixel, nx * ny <=
 *   RT_MAX_SAMPLES (else RT_ERR_INVALID), row-major with j outer: ox = (float)((i + 0.5) / nx - 0.5) computed in
 *   double, oy likewise from j and ny. 1 x 1 is the single offset (0, 0).
 * rt_sample_pattern_jittered(nx, ny, rng, out): the same cells with the 0.5 replaced by rt_rand(rng) / (RAND_MAX + 1.0),
 *   drawn for x and then for y, cell by cell in that order; rng NULL = a fresh generator with seed 1.
 * rt_render_views_ss(s, views, lights, n_lights, frame, pattern, hip_stream) and
 * rt_render_views_ss_lit(s, views, ls, frame, pattern, hip_stream): rt_render_views / rt_render_views_lit with the
 *   pattern. Everything documented there holds: outputs, stream semantics, n_views == 0, host-only scenes, the
 *   order of the checks, devices[0] for a multi-device scene. pattern is host memory, read before the call
 *   returns; it travels with the camera records (same staging buffer, same copy, same events). Further refusals,
 *   after the NULL-argument check: a NULL pattern, n_samples outside 1..RT_MAX_SAMPLES, an offset that is not
 *   finite or lies outside [-1, 1]: RT_ERR_INVALID; a launch of 2^26 or more one-wave blocks: RT_ERR_INVALID.
 *   Kernels: k_views_ss_loop -- rt_render_views' 8x8-pixel waves, each lane tracing its pixel's S samples in turn
 *   (any S; the block count is rt_render_views') -- or k_views_ss_packed -- a wave is 64 / S neighbouring pixels times
 *   S samples (S = 2, 4, 8, 16, 32, 64: pixel blocks of 8x4, 4x4, 4x2, 2x2, 2x1, 1x1; S times the blocks), the
 *   samples of a pixel summed across lanes in the order above. Both run trace_depth at every mode and depth. Which
 *   one a power-of-two S takes by default is measured; variant bit 33554432 selects the other. Every
 *   other S takes the loop.
 * rt_render_ss(s, cam, lights, n_lights, frame, pattern, out_rgb): one supersampled frame into host memory
 *   ([H][W][3]); a one-view batch on the scene's stream into a device buffer the scene owns, then the copy.
 *   Synchronous.
 * ------------------------------------------------------------------------------------------- */
#define RT_HAS_SUPERSAMPLING 1
#define RT_MAX_SAMPLES 64
typedef struct rt_sample_pattern {
  int32_t n_samples;
  float offsets[RT_MAX_SAMPLES][2];  /* (ox, oy) per sample, in pixels */
} rt_sample_pattern;
int rt_sample_pattern_grid(int32_t nx, int32_t ny, rt_sample_pattern* out);
int rt_sample_pattern_jittered(int32_t nx, int32_t ny, rt_rand_state* rng, rt_sample_pattern* out);
int rt_render_views_ss(rt_scene* s, const rt_view_batch* views, const rt_light* lights, int32_t n_lights,
                       const rt_frame* frame, const rt_sample_pattern* pattern, void* hip_stream);
int rt_render_views_ss_lit(rt_scene* s, const rt_view_batch* views, const rt_light_set* ls, const rt_frame* frame,
                           const rt_sample_pattern* pattern, void* hip_stream);
int rt_render_ss(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* frame,
                 const rt_sample_pattern* pattern, float* out_rgb);
/* The plan of a supersampled batch (host only; plan_views with its sample count). in[0..9] (n_in = 10):
 * rt_debug_view_plan's nine, then n_samples. out[0..9] (n_out = 10): rt_debug_view_plan's seven -- 0 says which of
 * rt_render_views' kernels the same batch without a pattern would run; the sample kernels run trace_depth under
 * either -- then 7 the layout (0 loop, 1 packed), 8 pixels per wave, 9 one-wave blocks per 16x16 tile. With
 * n_samples = 1 the first seven are rt_debug_view_plan's numbers. For a refused plan rt_last_error holds the reason.
 * Variant bits read: rt_debug_view_plan's, and 33554432 (the non-default layout of a power-of-two sample count). */
int rt_debug_sample_plan(const int64_t in[], int32_t n_in, int64_t out[], int32_t n_out);

/* createDebugRay (flyscene.cpp:129-173) without the GL cylinders: the camera ray through a
 * (float) mouse position and its reflection chain, up to max_depth segments; every segment carries the
 * first ray's traceRay colour; a miss ends the chain with a 10-unit segment. *n_out = segments written. */
typedef struct rt_ray_segment {
  float origin[3], direction[3];
  float length;
  float color[3];
} rt_ray_segment;
int rt_debug_ray(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, float mouse_x, float mouse_y,
                 int32_t max_depth, rt_ray_segment* out, int32_t* n_out);

/* ---------------------------------------------------------------------------------------------
 * Misc
 * ------------------------------------------------------------------------------------------- */
int rt_device_count(void);       /* 0 when no GPU is visible */
int rt_version(void);            /* RT_API_VERSION */
/* "librtamd api <N> gfx950 sources <hash>": the build's identity. rt_source_hash() is the hash alone:
 * SHA-256 (first 16 hex digits) of the product sources this library was built from (the csrc/ .hip,
 * .cpp and .h files and include/rt/rt_api.h, concatenated in sorted path order), so a record can show that
 * the binary it ran matches the tree it came from. */
const char* rt_version_string(void);
const char* rt_source_hash(void);
const char* rt_last_error(void); /* thread-local */

/* Verification hooks (tests only; never used by the render path): evaluate the Eigen-order float
 * primitives of rt_math.h on the host (rt_debug_math_host) or in a gfx950 kernel
 * (rt_debug_math_device) for n known-answer cases of op (tests/golden/eigen_kat.bin; op 17 = the
 * specular term's pow, in {x, y} -> out {pow}, checked against the host C library). */
int rt_debug_math_host(int32_t op, int32_t n, const float* in, float* out);
int rt_debug_math_device(int32_t op, int32_t n, const float* in, float* out);

/* Host-side check of the scene's acceleration structures (tests only): every triangle lies inside
 * each ancestor box of the binary tree, of the 4-wide quantised tree and of the fp32 4-wide tree (whose
 * per-octant child orders must be permutations), and every triangle record sits in exactly one leaf of
 * each. info[0..6] = binary nodes, binary depth, quantised nodes, quantised depth, triangles reached
 * (binary), triangles reached (quantised), violations (all three trees). RT_OK iff sound. */
int rt_debug_validate_bvh(const rt_scene* s, int64_t info[7]);
/* Surface-area cost of the binary tree (host data, tests and A/B only): out[0] = k_trav * (interior
 * node area sum) + (triangle-weighted leaf area sum), over the root's area -- the SAH estimate of the
 * node steps and triangle tests of a random ray; out[1] = its node term, out[2] = its triangle term,
 * out[3] = the mean leaf size. */
int rt_debug_tree_cost(const rt_scene* s, double k_trav, double out[4]);
/* Record layout of the device node allocation for a scene of n_nodes binary nodes, n_tris triangle
 * records and n_wide fp32 4-wide nodes per octant copy (host only, no device): out[0] = allocation bytes
 * (0: records exceed 4 GiB), out[1] = byte offset of the wide copies (0: the wide tree is dropped because
 * a wide record offset would reach 2^31, the leaf-handle bit). */
int rt_debug_record_layout(int64_t n_nodes, int64_t n_tris, int64_t n_wide, int64_t out[2]);
/* The dispatch plan of a frame (host only, no device; csrc/rt_dispatch.h plan_frame, which rt_render reads for
 * every kernel and block-order decision), with the dispatch knobs at their defaults.
 * in[0..10] (n_in = 11): mode, max_depth, flags, tiles_x, tiles_y (16x16-pixel tiles of the frame), shard_index,
 * shard_count (>= 1), kernel variant, bytes of the scene's binary node + triangle records, whether the scene has
 * the quantised 4-wide tree, whether no other frame of the scene is in flight. n_in = 12 adds in[11] = the number
 * of lights the frame reads from a light set in device memory (0 = none, the 11-input plan): non-zero selects the
 * generic-depth kernel for PRIMARY and FULL at every depth.
 * out[0..13] (n_out = 14): 0 kernel (0 none: empty shard, 1 generic depth, 2 PRIMARY fused, 3 PRIMARY trace +
 * shade, 4 PRIMARY dual, 5 PRIMARY two rays per lane, 6 PRIMARY persistent, 7 FULL megakernel, 8 FULL pipeline),
 * 1 traversal flavour (0 VGPR stack, 1 LDS stack, 2 quantised 4-wide), 2 needs the variants library, 3 the
 * shard's tile slots, 4 units (one-wave blocks of the render kernel), 5 recursion limit, 6 L2-resident scene,
 * 7 xcd_remap (run length of the chunked XCD block order; 1 contiguous per XCD, 0 plain), 8 the kernel writes
 * per-wave counts (else RT_FRAME_WAVE_STATS is refused), 9 dispatched longest-first, 10 ceiling of the waves
 * split into sub-waves once the frame has an order, 11 takes the next XCD band rotation, 12 binds the stage
 * pipeline's buffers (whole frames only), 13 FULL megakernel's small-scene build. */
int rt_debug_frame_plan(const int64_t in[], int32_t n_in, int32_t out[], int32_t n_out);
/* The accept path's shortcuts (host data, no device needed): counts[0] = triangle records, counts[1] =
 * those whose interpolated normal is certified non-zero, counts[2] = those with a reference-box
 * certificate; *cert_origin_max (may be NULL) = the object-space origin range (max norm) within which
 * certified faces skip the box predicate; face_flags (may be NULL, else n_faces entries) = per face the
 * OR of its records' flag bits (0x80000000 safe normal, 0x40000000 box certificate). */
int rt_debug_scene_flags(const rt_scene* s, int64_t counts[3], float* cert_origin_max, uint32_t* face_flags);

/* Kernel-variant override (tests and A/B measurements only; default 0 = the measured-best kernels).
 * Bits of the product library: 4 / 512 / 1536 tile orders, 8192 / 16384 FULL megakernel builds, 32768
 * PRIMARY as trace + shade kernels, 65536 the generic traceRay kernel, 131072 / 262144 / 524288
 * longest-first dispatch knobs (524288, longest-first also with frames in flight, is A/B only: the frames share
 * one order, which one of them may read while another's sort rewrites it, and then skip or repeat waves),
 * 2097152 PRIMARY packets on the binary tree, 4194304 the origin-major layout of the ray streams' coherence key
 * (rt_debug_ray_keys follows it), 8388608 light sets read from device memory at any count (by default only sets
 * beyond RT_MAX_LIGHTS are; lets the tests compare the two paths at 0, 1 and 32 lights; a set of 0 lights has no
 * light to read and keeps the default kernels), 16777216 the memory-lights kernels without the wave-level occluder
 * cache of their shadow packets (A/B and tests), 33554432 supersampled view batches in the layout that is not the
 * default at their sample count (power-of-two counts; A/B and tests). Bits of the variants library
 * only (make variants -> librtamd_variants.so; the product library's rt_render returns
 * RT_ERR_UNSUPPORTED for them): 1 VGPR wave stack, 2 4-wide quantised BVH (scenes of the host builders,
 * which also build that tree), 16 FULL as a stage pipeline (whole frames only: a sharded frame returns
 * RT_ERR_UNSUPPORTED) (+32/64/128 per-lane traversal in its reflection / secondary-shadow / primary-shadow
 * stages), 256 two
 * rays per lane, 2048 persistent threads (+4096 no stealing), 1048576 two packets per wave. Every
 * variant renders the same bits. Returns the previous value. */
int rt_debug_set_variant(int32_t v);
/* Diagnostics: on = 1 lets the library read its A/B and diagnostic environment knobs (RT_KERNEL_VARIANT,
 * RT_SPLIT_K, RT_SPLIT_KP, RT_TIMELINE_SPLIT, RT_LDS_PAD, RT_LPT_REFRESH, RT_LPT_MOVED,
 * RT_LPT_DILATE, RT_LPT_PRED, RT_ASM_DEVICE, RT_SLOT_POOL, RT_HWQ_GPU_CAP, RT_SAH_TRAV, RT_SBVH_BUDGET, RT_NODE_LAYOUT, RT_PLOC_RADIUS, RT_PLOC_TRAV, RT_PLOC_RULE, RT_TIMING); by default
 * (and after on = 0) it ignores the process environment, so a drop-in's trees, kernels and dispatch never
 * depend on it. Turning it on also takes RT_KERNEL_VARIANT as the current kernel variant. */
int rt_debug_env_knobs(int32_t on);

/* Wave timeline of the last frame rendered with RT_FRAME_TIMELINE (diagnostics): per wave, in dispatch
 * order (workgroup id), 8 words: shader-clock s_memtime at start (lo, hi) and end (lo, hi), the
 * constant 100 MHz s_memrealtime at start and end (low 32 bits), HW_ID, and XCC_ID << 28 | the logical
 * wave (tile * 4 + quarter) the block traced. *n_waves = waves of
 * that frame; capacity_waves smaller than that -> RT_ERR_INVALID. */
int rt_debug_timeline(rt_scene* s, int64_t capacity_waves, uint32_t* out8, int64_t* n_waves);

/* Raw counters of the last RT_FRAME_STATS frame (diagnostics), out[0..n): 0 node visits, 1 triangle tests,
 * 2 wave node fetches, 3 wave triangle fetches, 4 primary rays, 5 hits, 6 total rays, 7 wave stack pops,
 * 8 pops at which no lane that wanted the entry still could reach it before its closest hit (closest-hit
 * traversal only); 48..63: the FULL kernel's packet walks by phase (csrc/rt_traverse.h ST_PW .. ST_PH); entries past
 * the last counter are 0. */
int rt_debug_counters(rt_scene* s, int64_t n, int64_t* out);

/* Per-wave counts of the last frame rendered with RT_FRAME_STATS | RT_FRAME_WAVE_STATS (diagnostics), indexed by
 * logical wave (tile * 4 + quarter), 8 words each: PRIMARY node steps, triangle tests, hit lanes, 0 x 5; FULL the
 * node steps of its four packet phases (primary, shadows of the primary hits, reflection, shadows of the
 * reflection hits), then their triangle tests. *n_waves = the frame's logical waves; capacity_waves smaller than
 * that -> RT_ERR_INVALID. */
int rt_debug_wave_stats(rt_scene* s, int64_t capacity_waves, uint32_t* out8, int64_t* n_waves);

/* Longest-first dispatch of lone frames (diagnostics): out3[0] = lone frames dispatched with the scene's cost
 * map since the scene was created, out3[1] = of them, frames that re-sorted the map from their own wave costs
 * (a new frame shape, every 8th frame, or a camera moved since the map's frame), out3[2] = 1 when a valid map is
 * held. Device 0's replica for a multi-device scene. */
int rt_debug_lpt_stats(const rt_scene* s, int64_t* out3);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
