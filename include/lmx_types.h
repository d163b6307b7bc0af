/* lmx_types.h — plain-C POD layouts shared by the C ABI (lumix_mi355.h), the CPU oracle (oracle/) and tests.
 *
 * Every struct here is byte-compatible with the LumixEngine type it names, so an engine-side adapter can
 * reinterpret_cast instead of converting. Citations are relative to the reference tree (src/...).
 */
#ifndef LMX_TYPES_H
#define LMX_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Frustum plane slots, core/geometry.h:73-83 (Frustum::Planes). EXTRA0/EXTRA1 duplicate NEAR
 * (core/geometry.cpp:134-136, 343-345). */
enum {
	LMX_PLANE_NEAR = 0,
	LMX_PLANE_FAR = 1,
	LMX_PLANE_LEFT = 2,
	LMX_PLANE_RIGHT = 3,
	LMX_PLANE_TOP = 4,
	LMX_PLANE_BOTTOM = 5,
	LMX_PLANE_EXTRA0 = 6,
	LMX_PLANE_EXTRA1 = 7,
	LMX_PLANE_COUNT = 8
};

/* RenderableTypes, renderer/render_module.h:293-301. The u8 `type` of a culling cell / CullResult page. */
enum {
	LMX_TYPE_MESH = 0,
	LMX_TYPE_DECAL = 1,
	LMX_TYPE_LOCAL_LIGHT = 2,
	LMX_TYPE_CURVE_DECAL = 3,
	LMX_TYPE_PARTICLES = 4,
	LMX_TYPE_COUNT = 5,
	LMX_TYPE_ALL = 0xff /* culling_system.cpp:310-319: 0xff is reserved for "all types" */
};

/* ShiftedFrustum, core/geometry.h:102-153: 8 planes SoA + 8 corner points (fp32, relative to `origin`) + fp64 origin.
 * sizeof == 256, alignas(16). */
typedef struct LmxShiftedFrustum {
	float xs[LMX_PLANE_COUNT];
	float ys[LMX_PLANE_COUNT];
	float zs[LMX_PLANE_COUNT];
	float ds[LMX_PLANE_COUNT];
	float points[8][3];
	double origin[3];
	double _pad; /* alignas(16) tail padding of the reference struct */
} LmxShiftedFrustum;

/* Frustum, core/geometry.h:29-99 (the cell-relative result of ShiftedFrustum::getRelative). sizeof == 224. */
typedef struct LmxFrustum {
	float xs[LMX_PLANE_COUNT];
	float ys[LMX_PLANE_COUNT];
	float zs[LMX_PLANE_COUNT];
	float ds[LMX_PLANE_COUNT];
	float points[8][3];
} LmxFrustum;

/* Transform, core/math.h:306-327: fp64 position, fp32 quaternion (x,y,z,w), fp32 non-uniform scale. sizeof == 56. */
typedef struct LmxTransform {
	double pos[3];
	float rot[4];
	float scale[3];
	float _pad;
} LmxTransform;

/* LocalRigidTransform, core/math.h:262-270: fp32 position + quaternion. sizeof == 28. */
typedef struct LmxLocalRigidTransform {
	float pos[3];
	float rot[4];
} LmxLocalRigidTransform;

/* Matrix, core/math.h:329-393: column-major 4x4 fp32, columns[c] = {x,y,z,w}. sizeof == 64. */
typedef struct LmxMatrix {
	float columns[4][4];
} LmxMatrix;

/* Mesh::Skin, renderer/model.h:81-84. sizeof == 24. */
typedef struct LmxSkin {
	float weights[4];
	int16_t indices[4];
} LmxSkin;

/* Viewport, core/geometry.h:177-199 (only the fields Viewport::getFrustum() reads). Not layout-compatible. */
typedef struct LmxViewport {
	int32_t is_ortho;
	float fov;
	float ortho_size;
	int32_t w;
	int32_t h;
	double pos[3];
	float rot[4];
	float near_plane;
	float far_plane;
} LmxViewport;

enum {
	LMX_CULL_CELL_SIZE = 300,        /* culling_system.cpp:75 */
	LMX_CULL_PAGE_SPHERES = 201,     /* CellPage::MAX_COUNT, culling_system.cpp:59 */
	LMX_CULLRESULT_PAGE_IDS = 1020,  /* culling_system.h:55 */
	LMX_MAX_BONES = 196              /* Model::Bone::MAX_COUNT, renderer/model.h:155 */
};

/* ---- createSortKeys inputs (renderer/pipeline.cpp:3789-3968) ---- */

/* LODMeshIndices, renderer/model.h:129-133 */
typedef struct LmxLodIndices {
	int32_t from, to;
} LmxLodIndices;

/* The fields of Model that createSortKeys reads: m_lod_distances[MAX_LOD_COUNT] (squared distances, model.h:234),
 * m_lod_indices[MAX_LOD_COUNT + 1] (model.h:233; entry 4 stays {0, -1}, model.cpp:98) and Mesh::type of its meshes. */
typedef struct LmxKeysModel {
	float lod_distances[4];
	LmxLodIndices lod_indices[5];
	uint32_t first_mesh; /* into the mesh-type table of lmx_keys_set_models */
	uint32_t mesh_count;
} LmxKeysModel;

/* MeshMaterial (renderer/model.h:59-68) as createSortKeys sees it: sort_key and material->getLayer(). */
typedef struct LmxMeshMaterial {
	uint32_t sort_key;
	uint8_t layer;
	uint8_t _pad[3];
} LmxMeshMaterial;

enum { LMX_MESH_RIGID = 0, LMX_MESH_SKINNED = 1 };         /* Mesh::Type, renderer/model.h:86-89 */
enum { LMX_MODEL_INSTANCE_MOVED = 1 << 3 };                  /* ModelInstance::MOVED, renderer/render_module.h:212 */

/* DrawCommandTypes, renderer/pipeline.cpp:41-51 (bits 32..36 of a sort value) */
enum {
	LMX_DRAW_MESH = 0,
	LMX_DRAW_AUTOINSTANCED = 1,
	LMX_DRAW_SKINNED = 2,
	LMX_DRAW_DECAL = 3,
	LMX_DRAW_CURVE_DECAL = 4
};
#define LMX_SORT_KEY_BUCKET_SHIFT 56                         /* pipeline.cpp:70 */
#define LMX_SORT_KEY_INSTANCED_FLAG (1ull << 55)             /* pipeline.cpp:71 */
#define LMX_SORT_VALUE_INSTANCER_SHIFT 16                    /* pipeline.cpp:73 */
#define LMX_SORT_VALUE_MESH_IDX_SHIFT 40                     /* pipeline.cpp:76 */
#define LMX_SORT_VALUE_TYPE_SHIFT 32                         /* pipeline.cpp:77 */

/* The per-view state createSortKeys reads (pipeline.cpp:3797-3832). */
typedef struct LmxKeysView {
	double camera_pos[3];             /* view.cp.pos */
	double lod_ref_point[3];          /* m_viewport.pos */
	float lod_multiplier;             /* Renderer::getLODMultiplier() */
	float time_delta;                 /* Engine::getLastTimeDelta() */
	uint32_t frame_number;            /* Renderer::frameNumber() % 0xffFFffFF */
	uint8_t is_shadow;                /* view.cp.is_shadow */
	uint8_t layer_to_bucket[255];     /* View::layer_to_bucket, 0xff = no bucket renders the layer (pipeline.cpp:1003-1020) */
	uint8_t bucket_depth_sorted[256]; /* buckets[b].sort == BucketDesc::DEPTH */
} LmxKeysView;

/* ---- createCommands outputs (renderer/pipeline.cpp:2747-3320) ---- */

/* Kind of a run = DrawCommandTypes of its first pair; a MESH run whose head carries ModelInstance::MOVED is LMX_RUN_MOVED_MESH. */
enum {
	LMX_RUN_MESH = 0,          /* 48 B records: rot[4], lpos[3], lod_d, scale[3], material_index (:3098-3117) */
	LMX_RUN_AUTOINSTANCED = 1, /* no records of its own: the group's 48 B records lie in the group buffer (:3992-4010) */
	LMX_RUN_SKINNED = 2,       /* 92 B (:3146-3181) */
	LMX_RUN_DECAL = 3,         /* 52 B, front part / back part (:3202-3227) */
	LMX_RUN_CURVE_DECAL = 4,   /* 68 B (:3263-3290) */
	LMX_RUN_MOVED_MESH = 32    /* 96 B (:3053-3080); outside the 5 bits of a pair type, so no unhandled type can collide with it */
};

/* One run = one draw call of createCommands, in pair order. sizeof == 48. */
typedef struct LmxDrawRun {
	uint32_t kind;        /* LMX_RUN_* (a pair type lmx_keys_run never emits: that type, stride 0, one pair) */
	uint32_t bucket;      /* key >> 56 */
	uint32_t batch;       /* the slice of the pairs (substream) the run lies in */
	uint32_t first_pair, pair_count;
	uint32_t data_offset; /* bytes, 16-aligned: into the instance buffer; AUTOINSTANCED: into the group buffer (48 * offsets[group]) */
	uint32_t stride;      /* bytes per record */
	uint32_t head_entity; /* entity of the first pair; AUTOINSTANCED: of the group's first renderable (:3010-3011) */
	uint32_t mesh_idx;    /* of the first pair / of the group's first renderable */
	uint32_t front_count; /* decal runs: records [0, front_count) do not intersect the near plane, the rest do; else pair_count */
	uint32_t group;       /* AUTOINSTANCED: group index (mesh sort key) */
	uint32_t total_count; /* AUTOINSTANCED: records of the group; else pair_count */
} LmxDrawRun;

/* The per-view state createCommands reads: view.cp.pos, view.cp.frustum, buckets[b].sort == BucketDesc::DEPTH */
typedef struct LmxDrawView {
	double camera_pos[3];
	LmxShiftedFrustum frustum;
	uint8_t bucket_depth_sorted[256];
} LmxDrawView;

typedef struct LmxDrawCounts {
	uint32_t pairs;          /* pairs walked */
	uint32_t runs;
	uint32_t instance_bytes; /* bytes of the instance buffer in use (slices are 16-byte aligned) */
	uint32_t group_records;  /* 48-byte records in the group buffer (= the instancer CSR's total) */
	uint32_t overflow;       /* != 0: an output buffer was too small (never with library-sized buffers) */
} LmxDrawCounts;

/* ---- fillClusters inputs (renderer/pipeline.cpp:3387-3410) ---- */

/* PointLight (renderer/render_module.h:156-171) as fillClusters reads it, by entity index. sizeof == 32. */
typedef struct LmxPointLight {
	float color[3];
	float intensity;
	float range;
	float fov;
	float attenuation_param;
	uint32_t flags;
} LmxPointLight;

/* ---- animation sampling inputs (animation/animation.h:86-115, animation.cpp:29-204) ---- */

typedef struct LmxAnimConstTranslation { /* Animation::ConstTranslationTrack */
	float value[3];
	uint16_t bone_index;
	uint16_t _pad;
} LmxAnimConstTranslation;

typedef struct LmxAnimTranslationTrack { /* Animation::TranslationTrack: bit-packed, value = min + to_range * bits (in fp64, animation.cpp:313-316) */
	float min[3];
	float to_range[3];
	uint16_t offset_bits;
	uint16_t bone_index;
	uint8_t bitsizes[3];
	uint8_t _pad;
} LmxAnimTranslationTrack;

typedef struct LmxAnimConstRotation { /* Animation::ConstRotationTrack */
	float value[4];
	uint16_t bone_index;
	uint16_t _pad;
} LmxAnimConstRotation;

typedef struct LmxAnimRotationTrack { /* Animation::RotationTrack: 3 packed channels + sign bit, the skipped one rebuilt from the norm */
	float min[3];
	float to_range[3];
	uint16_t offset_bits;
	uint16_t bone_index;
	uint8_t bitsizes[3];
	uint8_t skipped_channel;
} LmxAnimRotationTrack;

/* What AnimationSampler reads of an Animation resource. Streams hold frame_count + 1 frames (animation.cpp:464), the root-motion arrays
 * frame_count + 1 entries; the library copies exactly those bits. The clip's end: the sample point is clamped to frame_count - 0.00001f,
 * which in fp32 is frame_count itself from 257 frames on, so a sample at or past the end of such a clip decodes frames frame_count and
 * frame_count + 1 (times f == 0) - in the engine, whatever lies behind the streams. Here the frame after the last reads as zero bits
 * (and the root-motion entry after the last as zeros); against the engine this can differ in the sign of a zero only.
 * lmx_anim_add refuses a clip whose frame_size_bits * (frame_count + 2) + 64 does not fit 32 bits, for either stream, and a frame_count
 * above 2^24 (there (float)frame_count can round up, and the clamp with it, past the frames a clip has). */
typedef struct LmxAnimation {
	float fps;                               /* m_fps */
	uint32_t frame_count;                    /* m_frame_count */
	uint32_t length;                         /* getLength().raw(): Time units of 1 / 32768 s (animation.h:41) */
	uint32_t translations_frame_size_bits;   /* m_translations_frame_size_bits */
	uint32_t rotations_frame_size_bits;      /* m_rotations_frame_size_bits */
	uint32_t n_const_translations, n_translations, n_const_rotations, n_rotations;
	const LmxAnimConstTranslation* const_translations;
	const LmxAnimTranslationTrack* translations;
	const LmxAnimConstRotation* const_rotations;
	const LmxAnimRotationTrack* rotations;
	const uint8_t* translation_stream;
	uint64_t translation_stream_size;
	const uint8_t* rotation_stream;
	uint64_t rotation_stream_size;
	int32_t root_translation_track;          /* RootMotion::translation_track_idx, -1 = none (animation.cpp:320) */
	int32_t root_rotation_track;             /* RootMotion::rotation_track_idx, -1 = none (animation.cpp:33) */
	const float* root_pose_translations;     /* RootMotion::pose_translations, (frame_count + 1) x 3 */
	const float* root_pose_rotations;        /* RootMotion::pose_rotations, (frame_count + 1) x 4 */
} LmxAnimation;

/* ---- animation clip compressor (lmx_animcomp_*, lumix_mi355.h "Animation compressor") ---- */

typedef struct LmxAnimKey { /* ModelImporter::Key: one bone at one sample */
	float pos[3];
	float rot[4];
} LmxAnimKey;

/* a clip's status: 0, or the smallest code that applies to it */
enum {
	LMX_ANIMCOMP_OK = 0,
	LMX_ANIMCOMP_NO_SAMPLES = 1,     /* n_samples == 0 */
	LMX_ANIMCOMP_BAD_ERROR = 2,      /* an error that is not finite and positive */
	LMX_ANIMCOMP_NONFINITE_BIND = 3, /* of a bone with keys */
	LMX_ANIMCOMP_NONFINITE_KEY = 4,
	LMX_ANIMCOMP_QUOTIENT_RANGE = 5, /* range / constant / error is 2^32 or more */
	LMX_ANIMCOMP_CHANNEL_BITS = 6,   /* a channel above 30 bits */
	LMX_ANIMCOMP_ENTRY_BITS = 7,     /* an entry above 57 bits (lmx_anim_add's limit) */
	LMX_ANIMCOMP_FRAME_BITS = 8      /* a frame above 65535 bits (offset_bits is 16 bits wide) */
};

typedef struct LmxAnimCompClip {
	uint32_t n_bones;              /* 1 .. LMX_MAX_BONES */
	uint32_t n_samples;
	float fps;                     /* not used by the compressor: carried for the file's header */
	float translation_error;       /* ModelMeta::anim_translation_error */
	float rotation_error;          /* ModelMeta::anim_rotation_error */
	uint32_t _pad;
	const uint8_t* has_keys;       /* n_bones bytes, 0: the bone's key array is empty; NULL: every bone has keys */
	const float* bind_positions;   /* n_bones x 3: each bone's local bind position */
	uint64_t key_offset;           /* of the clip's first record in `keys`; the clip holds n_samples x n_bones records, sample-major */
} LmxAnimCompClip;

typedef struct LmxAnimCompInfo {
	uint32_t n_const_translations, n_translations, n_const_rotations, n_rotations;
	uint32_t translations_frame_size_bits, rotations_frame_size_bits;
	uint64_t translation_stream_size, rotation_stream_size; /* bytes: (frame size x n_samples + 7) / 8 */
	uint32_t frame_count;          /* n_samples - 1 */
	uint32_t status;               /* LMX_ANIMCOMP_*; a refused clip has zero counts and sizes */
} LmxAnimCompInfo;

/* the caller's arrays lmx_animcomp_read_clip fills, shaped like LmxAnimation's; a NULL array is skipped */
typedef struct LmxAnimCompOutput {
	LmxAnimConstTranslation* const_translations;
	LmxAnimTranslationTrack* translations;
	LmxAnimConstRotation* const_rotations;
	LmxAnimRotationTrack* rotations;
	uint8_t* translation_stream;
	uint8_t* rotation_stream;
	uint32_t cap_tracks;           /* records each of the four tables has room for */
	uint32_t _pad;
	uint64_t cap_translation_stream, cap_rotation_stream; /* bytes */
} LmxAnimCompOutput;

/* One SAMPLE instruction of an Animator's blend stack (anim::BlendStackInstructions::SAMPLE, controller.cpp:282-289: slot, weight,
 * time, looped as the controller's nodes wrote them; `animation` is the id lmx_anim_add returned for RuntimeContext::animations[slot]). */
typedef struct LmxBlendSample {
	uint32_t animation;
	float weight;
	uint32_t time;                           /* Time units; wrapped (looped) or clamped to the animation's length by getPose, controller.cpp:148 */
	uint32_t looped;
} LmxBlendSample;

/* One instruction of an Animator's blend stack (anim::BlendStackInstructions, controller.h:58-62), in the controller's emission order. A
 * SAMPLE record carries the fields of LmxBlendSample. An IK record is what evalBlendStack hands evalIK (controller.cpp:275-281): `alpha` is
 * the caller's fp32 product alpha * RuntimeContext::weight, `leaf_bone` a bone index of the instance's model (LMX_BONE_NONE: the leaf was
 * not found in the model - the instruction does nothing, :180-183), `bones_count` the chain length in [1, LMX_IK_MAX_BONES]. sizeof == 48. */
#define LMX_BLEND_SAMPLE 1u
#define LMX_BLEND_IK 2u
#define LMX_BONE_NONE 0xffffffffu
#define LMX_IK_MAX_BONES 32                  /* evalIK's MAX_BONES_COUNT, controller.cpp:171 */
typedef struct LmxBlendInstr {
	uint32_t op;                             /* LMX_BLEND_SAMPLE or LMX_BLEND_IK */
	uint32_t animation;                      /* SAMPLE */
	float weight;
	uint32_t time;
	uint32_t looped;
	float alpha;                             /* IK */
	float target[3];
	uint32_t leaf_bone;
	uint32_t bones_count;
	uint32_t _pad;
} LmxBlendInstr;

#define LMX_TIME_ONE_SECOND (1u << 15)       /* Time::ONE_SECOND, animation/animation.h:41 */
#define LMX_ANIM_NONE 0xffffffffu

/* Animator controllers (anim::Controller). A controller's node tree may nest pose nodes LMX_CONTROLLER_MAX_POSE_DEPTH deep (a root
 * alone has depth 1) and a value tree may need LMX_CONTROLLER_MAX_VALUE_DEPTH operands at once (a chain of math nodes that deep). */
#define LMX_CONTROLLER_NONE 0xffffffffu
#define LMX_CONTROLLER_MAX_POSE_DEPTH 8
#define LMX_CONTROLLER_MAX_VALUE_DEPTH 8
#define LMX_ANIMATOR_USE_ROOT_MOTION 1u      /* Animator::USE_ROOT_MOTION, animation_module.cpp:46 */
#define LMX_VALUE_NUMBER 0u                  /* anim::Value::Type, controller.h:17-21 */
#define LMX_VALUE_BOOL 1u
#define LMX_VALUE_VEC3 2u

/* anim::Value (controller.h:16-37): an input of an Animator. A BOOL is its first byte, zero or not. sizeof == 16. */
typedef struct LmxAnimatorValue {
	uint32_t type;                           /* LMX_VALUE_* */
	union {
		float f;
		uint8_t b;
		float v3[3];
	};
} LmxAnimatorValue;

/* What lmx_anim_controller_check reports of a compiled controller resource. */
typedef struct LmxControllerInfo {
	uint32_t version;                        /* ControllerVersion of the header */
	uint32_t n_inputs;                       /* m_inputs */
	uint32_t n_slots;                        /* m_animation_slots_count */
	uint32_t n_entries;                      /* m_animation_entries */
	uint32_t n_nodes;                        /* pose nodes */
	uint32_t n_ik;                           /* IK nodes */
	uint32_t state_bytes;                    /* upper bound of RuntimeContext::data after any update */
	uint32_t max_instrs;                     /* upper bound of the blend instructions one update emits */
	uint32_t enter_bytes;                    /* RuntimeContext::data as Controller::createRuntime leaves it */
	uint32_t pose_depth, value_depth;        /* the nesting the tree uses of the two caps */
	uint32_t _pad;
} LmxControllerInfo;

/* One ray of lmx_rays_cast: Ray {origin, dir} (core/geometry.h) with what castRay(ray, ignored) carries besides. sizeof == 48. */
typedef struct LmxRay {
	double origin[3];
	float dir[3];                            /* normalised (getRaySphereIntersection asserts it) */
	float t_max;                             /* a hit counts when its t < t_max: +inf, or the t of a hit the caller already holds */
	int32_t ignore;                          /* entity whose hits are left out, -1: none */
	uint32_t _pad;
} LmxRay;
/* The nearest model-instance hit of a ray. A ray without one is all zero. sizeof == 24. */
typedef struct LmxRayHit {
	uint32_t is_hit;
	int32_t entity;
	uint32_t mesh;                           /* index into the model's mesh list (RayCastModelHit::mesh = &model->getMesh(mesh)) */
	uint32_t triangle;                       /* index within that mesh */
	float t;                                 /* world space: length(ray.origin - hit position) */
	float t_model;                           /* what Model::castRay returned, along the model-space ray */
} LmxRayHit;
/* The nearest instanced-model hit of a ray (RenderModuleImpl::castRayInstancedModels). A ray without one is all zero. sizeof == 32. */
typedef struct LmxRayImHit {
	uint32_t is_hit;
	int32_t entity;                          /* the InstancedModel's entity (lmx_rays_set_instanced_models) */
	uint32_t model;                          /* its lmx_im model id */
	uint32_t subindex;                       /* RayCastModelHit::subindex: the instance's index in the stored (grid) order */
	uint32_t mesh;                           /* index into the model's mesh list, as LmxRayHit::mesh */
	uint32_t triangle;                       /* index within that mesh */
	float t;                                 /* t_model * the instance's scale: what the reference returns as hit.t */
	float t_model;                           /* what Model::castRay returned, along the instance-space ray (its direction is not normalised) */
} LmxRayImHit;
/* What castRayProceduralGeometry (render_module.cpp:2650-2712) reads of one ProceduralGeometry. The arrays are read during
 * lmx_rays_set_procedural_geometries only. sizeof == 64. */
typedef struct LmxRayProcGeom {
	int32_t entity;
	uint32_t triangles;                      /* vertex_decl.primitive_type == gpu::PrimitiveType::TRIANGLES */
	float aabb_min[3];
	float aabb_max[3];
	const void* vertex_data;                 /* a position is the first 12 bytes at index * stride */
	uint32_t vertex_bytes;                   /* vertex_data.size(); 0: the geometry is kept and never cast */
	uint32_t stride;                         /* vertex_decl.getStride(), >= 12 */
	const void* index_data;
	uint32_t index_bytes;                    /* 0: not indexed; 2 or 4 */
	uint32_t index_count;                    /* getIndexCount() */
} LmxRayProcGeom;
/* What Terrain::castRay (terrain.cpp:474-535) reads of one Terrain. The texels are read during lmx_rays_set_terrains only. sizeof == 40. */
#define LMX_RAY_TERRAIN_R16 0u               /* gpu::TextureFormat::R16: 2 bytes per texel */
#define LMX_RAY_TERRAIN_RGBA8 1u             /* gpu::TextureFormat::RGBA8: 4 bytes per texel, the height is the lowest byte */
typedef struct LmxRayTerrain {
	int32_t entity;
	uint32_t width, height;                  /* m_width, m_height */
	uint32_t format;                         /* LMX_RAY_TERRAIN_* */
	float scale[3];                          /* m_scale */
	uint32_t ready;                          /* m_heightmap && m_heightmap->isReady(); 0: never hit */
	const void* texels;                      /* width * height texels, row z after row z - 1 */
} LmxRayTerrain;
/* castRayProceduralGeometry's result for a ray. A ray without a hit is all zero. sizeof == 20. */
typedef struct LmxRayPgHit {
	uint32_t is_hit;
	int32_t entity;
	uint32_t geom;                           /* index in the table of lmx_rays_set_procedural_geometries */
	uint32_t triangle;
	float t;                                 /* along the geometry-space ray, whose direction is not normalised: the world parameter */
} LmxRayPgHit;
/* Terrain::castRay's result for a (ray, terrain) pair. A pair without a hit is all zero. sizeof == 28. */
typedef struct LmxRayTerrainHit {
	uint32_t is_hit;
	int32_t entity;
	uint32_t terrain;                        /* index in the table of lmx_rays_set_terrains */
	int32_t hx, hz;                          /* the cell of the walk that was hit */
	uint32_t tri;                            /* 0: (p0, p1, p2), 1: (p0, p2, p3) */
	float t;
} LmxRayTerrainHit;
/* RenderModuleImpl::castRay's result for a ray (render_module.cpp:2718-2775). A ray without a hit is all zero. sizeof == 24. */
#define LMX_RAY_HIT_MODEL_INSTANCE 1u        /* index = mesh, sub = triangle (LmxRayHit) */
#define LMX_RAY_HIT_INSTANCED_MODEL 2u       /* index = lmx_im model, sub = subindex (LmxRayImHit) */
#define LMX_RAY_HIT_PROCEDURAL_GEOM 3u       /* index = geometry, sub = triangle (LmxRayPgHit) */
#define LMX_RAY_HIT_TERRAIN 4u               /* index = terrain, sub = hz * width + hx (LmxRayTerrainHit) */
typedef struct LmxRaySceneHit {
	uint32_t is_hit;
	uint32_t component;                      /* LMX_RAY_HIT_* */
	int32_t entity;
	uint32_t index;
	uint32_t sub;
	float t;
} LmxRaySceneHit;

/* ---- terrain grass: Terrain::createGrass (renderer/terrain.cpp:26-139) and the quad loop of PipelineImpl::renderGrass
 * (renderer/pipeline.cpp:2119-2209) ---- */
#define LMX_GRASS_ROTATION_Y_UP 0u           /* GrassRotationMode::Y_UP */
#define LMX_GRASS_ROTATION_ALL_RANDOM 1u     /* GrassRotationMode::ALL_RANDOM */
enum {
	LMX_GRASS_MAX_TERRAINS = 64,
	LMX_GRASS_MAX_TYPES = 16,                /* per terrain: (splat >> 16) holds 16 bits, a type past them is never accepted */
	LMX_GRASS_SAMPLES = 1024,                /* iterations per quad */
	LMX_GRASS_SLOT_INSTANCES = 2048          /* records of one pool slot: every accepted sample is stored twice */
};
/* Terrain::GrassType. sizeof == 16. */
typedef struct LmxGrassType {
	float spacing;                           /* m_spacing; <= 0: createGrass skips the type */
	float distance;                          /* m_distance */
	uint32_t rotation_mode;                  /* LMX_GRASS_ROTATION_* */
	uint32_t usable;                         /* m_grass_model && m_grass_model->isReady(): 0 = renderGrass skips the type */
} LmxGrassType;
/* One terrain of lmx_grass_set_terrains; every array is copied at the call. sizeof == 80. */
typedef struct LmxGrassTerrain {
	LmxRayTerrain heightmap;                 /* entity, m_width / m_height, format, m_scale, ready, texels */
	uint32_t splat_width, splat_height;
	uint32_t splat_format;                   /* LMX_RAY_TERRAIN_RGBA8, or anything else: getPixelNearest gives 0 (texture.cpp:90-95) */
	uint32_t splat_ready;                    /* m_splatmap && m_splatmap->isReady(); 0: createGrass does nothing */
	const void* splat_texels;                /* RGBA8 texels; NULL (`data.empty()`): nothing is accepted */
	const LmxGrassType* types;
	uint32_t n_types;
	uint32_t _pad;
} LmxGrassTerrain;
/* One instance of a quad as the reference's vertex buffer holds it. sizeof == 32. */
typedef struct LmxGrassInstance {
	float position[3];
	float scale;
	float rotation[4];
} LmxGrassInstance;
/* Terrain::GrassQuad. An empty quad has instances_count 0 and aabb (FLT_MAX, -FLT_MAX). sizeof == 48. */
typedef struct LmxGrassQuad {
	float aabb_min[3], aabb_max[3];
	int32_t ij[2];
	uint32_t type;
	uint32_t instances_count;                /* twice the accepted samples */
	uint32_t terrain;                        /* index in the table of lmx_grass_set_terrains */
	uint32_t slot;                           /* the quad's slice of the pool: LMX_GRASS_SLOT_INSTANCES records from slot * LMX_GRASS_SLOT_INSTANCES */
} LmxGrassQuad;
/* A view of renderGrass. sizeof == 288. */
typedef struct LmxGrassView {
	LmxShiftedFrustum frustum;               /* cp.frustum */
	double viewport_pos[3];                  /* m_viewport.pos: the pipeline's main viewport, also for shadow views */
	float lod_multiplier;                    /* Renderer::getLODMultiplier */
	uint32_t _pad;
} LmxGrassView;
/* One drawIndexedInstanced of renderGrass's quad loop (per mesh of LOD 0 the engine replays it). sizeof == 24. */
typedef struct LmxGrassDraw {
	uint32_t quad;                           /* index in the live-quad list (lmx_grass_read_quads) */
	uint32_t slot;
	uint32_t terrain, type;
	uint32_t instance_count;
	float distance;                          /* drawcall_data.dist */
} LmxGrassDraw;
/* What renderGrass pushes to the profiler, per view and per mesh. sizeof == 16. */
typedef struct LmxGrassCounts {
	uint32_t draws;                          /* "Quad count" */
	uint32_t culled;                         /* "Culled" */
	uint32_t instances;                      /* "Instances" */
	uint32_t live;                           /* live quads the launch went over */
} LmxGrassCounts;

#ifdef __cplusplus
}
#endif

#endif
