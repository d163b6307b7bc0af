"""ctypes binding of liblumix_mi355.so (include/lumix_mi355.h) + thin host classes that mirror the reference's
interfaces for the hot path (names and argument meaning follow the C++ originals):

* :class:`CullingSystem`  — src/renderer/culling_system.h:58-77 (`add`, `remove`, `set`, `setPosition`, `setRadius`,
  `getRadius`, `isAdded`, `cull`)
* :class:`World`          — the transform/hierarchy subset of src/engine/world.h:49-209 in its batch form
* :class:`Skinning`       — Pose::computeAbsolute + computeSkinMatrices + evaluateSkin (src/renderer/pose.cpp,
  src/renderer/model.cpp:103-137) over many instances

This module is plumbing for tests and bench.py; a LumixEngine build binds the same C ABI from C++.
It never computes anything on the CPU: if the library or a gfx950 device is missing, it raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LMX_LIB_PATH") or os.path.join(PKG, "liblumix_mi355.so")  # LMX_LIB_PATH: tools/ sweeps over kernel build variants

MAX_FRUSTA, MAX_TYPES, MAX_VIEWS = 8, 8, 8
TYPE_ALL = 0xFF
CULL_OPT_TILE_VARIANT, CULL_OPT_MAX_SHARDS, CULL_OPT_COUNTER_PAD, CULL_OPT_AUTO_COMPACTION, CULL_OPT_DEVICE_OWNS_BOUND, CULL_OPT_OVERFLOW_RESERVE, CULL_OPT_ASYNC_COMPACTION, CULL_OPT_COMPACTION_MIN, CULL_OPT_MAP_ZERO_COPY = 0, 2, 3, 4, 5, 6, 7, 8, 9  # (1: retired)
KEYS_OPT_SLOT_ORDER, KEYS_OPT_SPLIT_STATE, KEYS_OPT_WALK_SHARDS, KEYS_OPT_BLOCK_RANKS = 0, 1, 2, 3
WORLD_OPT_FUSED_LEVELS = 0
SKIN_OPT_INSTANCES_PER_BLOCK = 0
SKIN_INSTANCES_PER_BLOCK_DEFAULT = 2  # what a fresh context uses (lmx_context.h: SkinState::multi)
(K_CULL_CLASSIFY, K_CULL_SPHERES, K_XFORM_LEVEL, K_SPHERE_REFRESH, K_POSE_PALETTE, K_SKIN_VERTICES, K_CULL_DYNAMIC) = range(7)
KERNEL_NAMES = ["cull_classify", "cull_spheres", "xform_level", "sphere_refresh", "pose_palette", "skin_vertices", "cull_dynamic", "sort_keys", "anim_update", "cull_patch",
                "pose_slices", "animators_update", "animators_pack"]
K_CULL_PATCH = 9
K_POSE_SLICES = 10

SHIFTED_FRUSTUM = np.dtype(
    [("xs", "<f4", 8), ("ys", "<f4", 8), ("zs", "<f4", 8), ("ds", "<f4", 8), ("points", "<f4", (8, 3)), ("origin", "<f8", 3), ("_pad", "<f8")],
    align=True,
)
TRANSFORM = np.dtype([("pos", "<f8", 3), ("rot", "<f4", 4), ("scale", "<f4", 3), ("_pad", "<f4")], align=True)
LOCAL_RIGID = np.dtype([("pos", "<f4", 3), ("rot", "<f4", 4)], align=True)
MATRIX = np.dtype([("columns", "<f4", (4, 4))], align=True)
SKIN = np.dtype([("weights", "<f4", 4), ("indices", "<i2", 4)], align=True)
ANIM_CONST_TRANSLATION = np.dtype([("value", "<f4", 3), ("bone_index", "<u2"), ("_pad", "<u2")], align=True)
ANIM_TRANSLATION_TRACK = np.dtype([("min", "<f4", 3), ("to_range", "<f4", 3), ("offset_bits", "<u2"), ("bone_index", "<u2"), ("bitsizes", "u1", 3), ("_pad", "u1")], align=True)
ANIM_CONST_ROTATION = np.dtype([("value", "<f4", 4), ("bone_index", "<u2"), ("_pad", "<u2")], align=True)
BLEND_SAMPLE = np.dtype([("animation", "<u4"), ("weight", "<f4"), ("time", "<u4"), ("looped", "<u4")], align=True)  # LmxBlendSample
BLEND_INSTR = np.dtype([("op", "<u4"), ("animation", "<u4"), ("weight", "<f4"), ("time", "<u4"), ("looped", "<u4"), ("alpha", "<f4"), ("target", "<f4", 3),
                        ("leaf_bone", "<u4"), ("bones_count", "<u4"), ("_pad", "<u4")], align=True)  # LmxBlendInstr
BLEND_SAMPLE_OP, BLEND_IK_OP, BONE_NONE, IK_MAX_BONES, ANIM_NONE = 1, 2, 0xFFFFFFFF, 32, 0xFFFFFFFF  # LMX_BLEND_*, LMX_BONE_NONE, LMX_IK_MAX_BONES, LMX_ANIM_NONE
ANIM_ROTATION_TRACK = np.dtype([("min", "<f4", 3), ("to_range", "<f4", 3), ("offset_bits", "<u2"), ("bone_index", "<u2"), ("bitsizes", "u1", 3), ("skipped_channel", "u1")],
                               align=True)
ANIMATOR_VALUE = np.dtype([("type", "<u4"), ("v", "<u4", 3)])  # LmxAnimatorValue: the union as three words (a NUMBER's bits, a BOOL's byte, a VEC3)
CONTROLLER_INFO = np.dtype([(k, "<u4") for k in ("version", "n_inputs", "n_slots", "n_entries", "n_nodes", "n_ik", "state_bytes", "max_instrs", "enter_bytes",
                                                    "pose_depth", "value_depth", "_pad")])
CONTROLLER_NONE = 0xFFFFFFFF
ANIMATOR_USE_ROOT_MOTION = 1
VALUE_NUMBER, VALUE_BOOL, VALUE_VEC3 = 0, 1, 2


class LmxAnimation(C.Structure):
    """LmxAnimation of include/lmx_types.h."""
    _fields_ = [("fps", C.c_float), ("frame_count", C.c_uint32), ("length", C.c_uint32), ("translations_frame_size_bits", C.c_uint32),
                ("rotations_frame_size_bits", C.c_uint32), ("n_const_translations", C.c_uint32), ("n_translations", C.c_uint32),
                ("n_const_rotations", C.c_uint32), ("n_rotations", C.c_uint32), ("const_translations", C.c_void_p), ("translations", C.c_void_p),
                ("const_rotations", C.c_void_p), ("rotations", C.c_void_p), ("translation_stream", C.c_void_p), ("translation_stream_size", C.c_uint64),
                ("rotation_stream", C.c_void_p), ("rotation_stream_size", C.c_uint64), ("root_translation_track", C.c_int32),
                ("root_rotation_track", C.c_int32), ("root_pose_translations", C.c_void_p), ("root_pose_rotations", C.c_void_p)]


def animation_struct(a: dict):
    """(LmxAnimation, keep-alive list) from a lumixengine_amd.scenes.animation dict. Optional keys translation_stream_size /
    rotation_stream_size declare fewer bytes than the arrays hold (default: all of them)."""
    keep = [np.ascontiguousarray(a["const_translations"], ANIM_CONST_TRANSLATION), np.ascontiguousarray(a["translations"], ANIM_TRANSLATION_TRACK),
            np.ascontiguousarray(a["const_rotations"], ANIM_CONST_ROTATION), np.ascontiguousarray(a["rotations"], ANIM_ROTATION_TRACK),
            np.ascontiguousarray(a["translation_stream"], np.uint8), np.ascontiguousarray(a["rotation_stream"], np.uint8),
            np.ascontiguousarray(a["root_pose_translations"], np.float32), np.ascontiguousarray(a["root_pose_rotations"], np.float32)]
    st = LmxAnimation(float(a["fps"]), int(a["frame_count"]), int(a["length"]), int(a["translations_frame_size_bits"]), int(a["rotations_frame_size_bits"]),
                      len(keep[0]), len(keep[1]), len(keep[2]), len(keep[3]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]),
                      int(a.get("translation_stream_size", len(keep[4]))), _ptr(keep[5]), int(a.get("rotation_stream_size", len(keep[5]))), int(a["root_translation_track"]), int(a["root_rotation_track"]), _ptr(keep[6]), _ptr(keep[7]))
    return st, keep


LOD_INDICES = np.dtype([("from", "<i4"), ("to", "<i4")])
KEYS_MODEL = np.dtype([("lod_distances", "<f4", 4), ("lod_indices", LOD_INDICES, 5), ("first_mesh", "<u4"), ("mesh_count", "<u4")], align=True)
MESH_MATERIAL = np.dtype([("sort_key", "<u4"), ("layer", "u1"), ("_pad", "u1", 3)], align=True)
KEYS_VIEW = np.dtype(
    [("camera_pos", "<f8", 3), ("lod_ref_point", "<f8", 3), ("lod_multiplier", "<f4"), ("time_delta", "<f4"), ("frame_number", "<u4"), ("is_shadow", "u1"),
     ("layer_to_bucket", "u1", 255), ("bucket_depth_sorted", "u1", 256)],
    align=True,
)
KEYS_COUNTS = np.dtype([("pairs", "<u4"), ("instanced", "<u4"), ("groups", "<u4"), ("poses", "<u4"), ("dirty", "<u4"), ("overflow", "<u4")])
DRAW_RUN = np.dtype([(k, "<u4") for k in ("kind", "bucket", "batch", "first_pair", "pair_count", "data_offset", "stride", "head_entity", "mesh_idx", "front_count",
                                          "group", "total_count")])  # LmxDrawRun
DRAW_VIEW = np.dtype([("camera_pos", "<f8", 3), ("frustum", SHIFTED_FRUSTUM), ("bucket_depth_sorted", "u1", 256)], align=True)  # LmxDrawView
DRAW_COUNTS = np.dtype([("pairs", "<u4"), ("runs", "<u4"), ("instance_bytes", "<u4"), ("group_records", "<u4"), ("overflow", "<u4")])
POSES_COUNTS = np.dtype([("instances", "<u4"), ("bytes", "<u4"), ("skipped", "<u4"), ("overflow", "<u4")])  # LmxPosesCounts
POSES_GUARD_BYTES = 256  # behind the frame's buffer (lmx_poses_read_buffer)
# the launch geometry of pose_kernels.hip (lmx_kernels.h; tests/test_pose_constants.py holds the two together): threads per block, blocks of
# the two slice steps - each owns a contiguous part of the list - and blocks of the dual-quaternion step (POSE_BLOCK / 64 waves each)
POSE_BLOCK, POSE_GRID, POSE_DQ_GRID = 256, 256, 1024
# fillClusters (lmx_clusters_*): table records, the view, the counters and the output records of renderer/pipeline.cpp:3331-3366
POINT_LIGHT = np.dtype([("color", "<f4", 3), ("intensity", "<f4"), ("range", "<f4"), ("fov", "<f4"), ("attenuation_param", "<f4"), ("flags", "<u4")])  # LmxPointLight
ENV_PROBE = np.dtype([("inner_range", "<f4", 3), ("outer_range", "<f4", 3), ("flags", "<u4"), ("sh_coefs", "<f4", (9, 3))])  # LmxEnvProbe
REFL_PROBE = np.dtype([("half_extents", "<f4", 3), ("texture_id", "<u4"), ("flags", "<u4")])  # LmxReflProbe
PROBE_ENABLED = 1 << 2
CLUSTER_PLANES = np.dtype([("size", "<u4", 3), ("_pad", "<u4"), ("xplanes", "<f4", (65, 4)), ("yplanes", "<f4", (65, 4)), ("zplanes", "<f4", (17, 4))])  # LmxClusterPlanes
CLUSTER_VIEW = np.dtype([("camera_pos", "<f8", 3), ("frustum", SHIFTED_FRUSTUM), ("viewport_w", "<u4"), ("viewport_h", "<u4")], align=True)  # LmxClusterView
CLUSTERS_COUNTS = np.dtype([("lights", "<u4"), ("env_probes", "<u4"), ("refl_probes", "<u4"), ("map_entries", "<u4"), ("overflow", "<u4")])  # LmxClustersCounts
CLUSTER_LIGHT = np.dtype([("pos", "<f4", 3), ("radius", "<f4"), ("rot", "<f4", 4), ("color", "<f4", 3), ("attenuation_param", "<f4"), ("atlas_idx", "<u4"), ("fov", "<f4"),
                          ("padding", "<f4", 2)])  # ClusterLight, 64 B
CLUSTER = np.dtype([("offset", "<u4"), ("lights_count", "<u4"), ("env_probes_count", "<u4"), ("refl_probes_count", "<u4")])
CLUSTER_ENV_PROBE = np.dtype([("pos", "<f4", 3), ("pad0", "<f4"), ("rot", "<f4", 4), ("inner_range", "<f4", 3), ("pad1", "<f4"), ("outer_range", "<f4", 3), ("pad2", "<f4"),
                              ("sh_coefs", "<f4", (9, 4))])  # 208 B
CLUSTER_REFL_PROBE = np.dtype([("pos", "<f4", 3), ("layer", "<u4"), ("rot", "<f4", 4), ("half_extents", "<f4", 3), ("pad1", "<f4")])  # 48 B
CLUSTERS_GUARD_BYTES = 256  # behind the light records, their entities and the map (lmx_clusters_read_*)
CLUSTER_MAX_PROBES = 1024
RAY = np.dtype([("origin", "<f8", 3), ("dir", "<f4", 3), ("t_max", "<f4"), ("ignore", "<i4"), ("_pad", "<u4")])  # LmxRay
RAY_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("mesh", "<u4"), ("triangle", "<u4"), ("t", "<f4"), ("t_model", "<f4")])  # LmxRayHit
RAY_MODEL = np.dtype([("aabb_min", "<f4", 3), ("aabb_max", "<f4", 3), ("origin_radius", "<f4"), ("ready", "<u4"), ("first_mesh", "<u4"), ("mesh_count", "<u4"),
                      ("lod0_from", "<u4")])  # LmxRayModel
RAY_IM_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("model", "<u4"), ("subindex", "<u4"), ("mesh", "<u4"), ("triangle", "<u4"), ("t", "<f4"),
                       ("t_model", "<f4")])  # LmxRayImHit
RAYS_IM_COUNTS = np.dtype([("rays", "<u4"), ("candidates", "<u4"), ("overflow", "<u4")])  # LmxRaysImCounts
RAYS_COUNTS = np.dtype([("rays", "<u4"), ("candidates", "<u4"), ("overflow", "<u4")])  # LmxRaysCounts
RAY_PROC_GEOM = np.dtype([("entity", "<i4"), ("triangles", "<u4"), ("aabb_min", "<f4", 3), ("aabb_max", "<f4", 3), ("vertex_data", "<u8"), ("vertex_bytes", "<u4"), ("stride", "<u4"),
                          ("index_data", "<u8"), ("index_bytes", "<u4"), ("index_count", "<u4")])  # LmxRayProcGeom (the pointers as addresses)
RAY_TERRAIN = np.dtype([("entity", "<i4"), ("width", "<u4"), ("height", "<u4"), ("format", "<u4"), ("scale", "<f4", 3), ("ready", "<u4"), ("texels", "<u8")])  # LmxRayTerrain
RAY_PG_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("geom", "<u4"), ("triangle", "<u4"), ("t", "<f4")])  # LmxRayPgHit
RAY_TERRAIN_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("terrain", "<u4"), ("hx", "<i4"), ("hz", "<i4"), ("tri", "<u4"), ("t", "<f4")])  # LmxRayTerrainHit
RAY_SCENE_HIT = np.dtype([("is_hit", "<u4"), ("component", "<u4"), ("entity", "<i4"), ("index", "<u4"), ("sub", "<u4"), ("t", "<f4")])  # LmxRaySceneHit
RAYS_SCENE_COUNTS = np.dtype([("rays", "<u4"), ("candidates", "<u4"), ("overflow", "<u4")])  # LmxRaysSceneCounts
RAY_TERRAIN_R16, RAY_TERRAIN_RGBA8 = 0, 1  # LMX_RAY_TERRAIN_*
RAY_HIT_MODEL_INSTANCE, RAY_HIT_INSTANCED_MODEL, RAY_HIT_PROCEDURAL_GEOM, RAY_HIT_TERRAIN = 1, 2, 3, 4  # LMX_RAY_HIT_*
RAY_CANDIDATE = np.dtype([("ray", "<u4"), ("entity", "<u4"), ("o", "<f4", 3), ("d", "<f4", 3), ("model", "<u4"), ("palette_at", "<u4"), ("n_bones", "<u4"), ("pad", "<u4")])  # 48 B
RAYS_GUARD_BYTES = 288  # behind the candidate list (lmx_rays_read_candidates)
RAY_INSTANCE_ENABLED, RAY_INSTANCE_VALID = 1 << 1, 1 << 2  # ModelInstance::Flags
# launch geometry of ray_kernels.hip (lmx_kernels.h; tests/test_ray_constants.py holds the two together)
RAY_BLOCK = 256
RAY_BROAD_RAYS = 64
RAY_BROAD_GRID = 2048
RAY_RUN = 4
RAY_NARROW_SPLIT = 4
RAY_NARROW_GRID = 4096
RAY_MAX_BONES = 256
# the instanced-model stage (k_imray_*; tests/test_ray_im_constants.py)
RAY_IM_BROAD_GRID = 2048
# ray_scene_kernels.hip (tests/test_ray_scene_constants.py)
RAY_PG_BROAD_GRID = 1024
RAY_TERRAIN_CHUNK = 64
RAY_TERRAIN_GRID = 2048
RAY_MAX_TERRAINS = 1024
RAYS_PG_OVERFLOW = 4  # bit of LmxRaysCounts::overflow
IM_TILE = 8192  # lmx_im.h: a model's slots start on a multiple of it
# the launch geometry of cluster_kernels.hip (lmx_kernels.h; tests/test_cluster_constants.py holds the two together): threads per block = the
# light tile of the gather, blocks of the record step that stride over the list, blocks of the count / fill steps
CLUSTER_BLOCK, CLUSTER_REC_GRID, CLUSTER_GRID = 256, 256, 1024
RUN_MESH, RUN_AUTOINSTANCED, RUN_SKINNED, RUN_DECAL, RUN_CURVE_DECAL, RUN_MOVED_MESH = 0, 1, 2, 3, 4, 32
VIEWPORT = np.dtype(
    [("is_ortho", "<i4"), ("fov", "<f4"), ("ortho_size", "<f4"), ("w", "<i4"), ("h", "<i4"), ("pos", "<f8", 3), ("rot", "<f4", 4), ("near_plane", "<f4"), ("far_plane", "<f4")],
    align=True,
)

# every symbol include/lumix_mi355.h declares: (name, restype, argtypes)
_vp, _u32, _i32, _u8, _f32, _ci, _sz = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint8, C.c_float, C.c_int, C.c_size_t
SYMBOLS = {
    "lmx_ctx_create": (_ci, [_ci, C.POINTER(_vp)]),
    "lmx_ctx_destroy": (None, [_vp]),
    "lmx_ctx_acquire_shared": (_ci, [_vp, _ci, C.POINTER(_vp)]),
    "lmx_ctx_release_shared": (None, [_vp]),
    "lmx_ctx_lock": (None, [_vp]),
    "lmx_ctx_unlock": (None, [_vp]),
    "lmx_last_error": (C.c_char_p, [_vp]),
    "lmx_ctx_set_stream": (_ci, [_vp, _vp]),
    "lmx_ctx_synchronize": (_ci, [_vp]),
    "lmx_profile_enable": (_ci, [_vp, _ci]),
    "lmx_profile_reset": (_ci, [_vp]),
    "lmx_profile_get": (_ci, [_vp, _ci, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "lmx_cull_build": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "lmx_cull_add": (_ci, [_vp, _i32, _u8, _vp, _f32]),
    "lmx_cull_remove": (_ci, [_vp, _i32]),
    "lmx_cull_set": (_ci, [_vp, _i32, _vp, _f32]),
    "lmx_cull_set_position": (_ci, [_vp, _i32, _vp]),
    "lmx_cull_set_radius": (_ci, [_vp, _i32, _f32]),
    "lmx_cull_get_radius": (_ci, [_vp, _i32, C.POINTER(_f32)]),
    "lmx_cull_is_added": (_ci, [_vp, _i32]),
    "lmx_cull_flush": (_ci, [_vp]),
    "lmx_cull_add_many": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "lmx_cull_set_many": (_ci, [_vp, _u32, _vp, _vp, _vp]),
    "lmx_cull_remove_many": (_ci, [_vp, _u32, _vp]),
    "lmx_cull_compact": (_ci, [_vp]),
    "lmx_cull_update_stats": (_ci, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "lmx_cull_async_stats": (_ci, [_vp, C.POINTER(_ci), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lmx_cull_set_option": (_ci, [_vp, _ci, _ci]),
    "lmx_cull_read_all": (_ci, [_vp, _u32, _u32, _vp, _u32, _vp]),
    "lmx_cull_map_all": (_ci, [_vp, _u32, _u32, _vp, _vp]),
    "lmx_cull_map_many": (_ci, [_vp, _u32, _u32, _vp, _vp]),
    "lmx_cull_map_begin": (_ci, [_vp, _u32, _u32]),
    "lmx_cull_map_end": (_ci, [_vp, _u32, _u32, _vp, _vp]),
    "lmx_cull_view_acquire": (_ci, [_vp, _vp, _u32]),
    "lmx_cull_view_release": (_ci, [_vp, _u32]),
    "lmx_cull_pack_device": (_ci, [_vp, _u32, _u32, _vp, _vp]),
    "lmx_cull_device_shards": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_cull_stats": (_ci, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "lmx_cull_layout_info": (_ci, [_vp, C.POINTER(_u32), C.POINTER(C.c_uint64)]),
    "lmx_cull": (_ci, [_vp, _u32, _vp, _u32, _u8]),
    "lmx_cull_set_pass_width": (_ci, [_vp, _u32]),
    "lmx_cull_counts": (_ci, [_vp, _u32, _vp]),
    "lmx_cull_read": (_ci, [_vp, _u32, _u32, _u8, _vp, _u32, C.POINTER(_u32)]),
    "lmx_cull_bind_output": (_ci, [_vp, _u32, _vp, _sz, _vp]),
    "lmx_cull_device_result": (_ci, [_vp, _u32, _u32, C.POINTER(_vp), C.POINTER(_vp), _vp, C.POINTER(_u32)]),
    "lmx_exchange_unique_id": (_ci, [_vp]),
    "lmx_exchange_create": (_ci, [_vp, _ci, _ci, _vp, _u32, C.POINTER(_vp)]),
    "lmx_exchange_destroy": (None, [_vp]),
    "lmx_exchange_cull": (_ci, [_vp, _vp, _u8, C.POINTER(_u32)]),
    "lmx_exchange_cull_many": (_ci, [_vp, _vp, _u32, _u8, C.POINTER(_u32)]),
    "lmx_exchange_read_many": (_ci, [_vp, _u32, _ci, _u32, _vp, _vp, _u32]),
    "lmx_exchange_wait": (_ci, [_vp, _u32]),
    "lmx_exchange_result": (_ci, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_vp)]),
    "lmx_exchange_read": (_ci, [_vp, _u32, _ci, _vp, _vp, _u32]),
    "lmx_exchange_info": (_ci, [_vp, _vp, _vp, _vp]),
    "lmx_exchange_set_caps": (_ci, [_vp, _u32, _vp, _ci]),
    "lmx_exchange_time_gather": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_exchange_layout": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "lmx_exchange_stats": (_ci, [_vp, _u32, _vp]),
    "lmx_world_build": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_world_build_with_world": (_ci, [_vp, _u32, _vp, _vp, _vp]),
    "lmx_world_set_parent": (_ci, [_vp, _i32, _i32]),
    "lmx_world_edit": (_ci, [_vp, _u32, _vp, _u32, _vp, _vp, _u32, _vp, _vp]),
    "lmx_world_info": (_ci, [_vp, _vp]),
    "lmx_world_read_local_transforms": (_ci, [_vp, _vp, _u32]),
    "lmx_transform_compose": (_ci, [_vp, _vp, _vp]),
    "lmx_transform_compute_local": (_ci, [_vp, _vp, _vp]),
    "lmx_world_set_transforms": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_world_set_world_transforms": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_world_set_transforms_device": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_world_bind_culling": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_world_propagate": (_ci, [_vp]),
    "lmx_world_read_transforms": (_ci, [_vp, _vp, _u32]),
    "lmx_world_set_option": (_ci, [_vp, _ci, _ci]),
    "lmx_world_track_moved": (_ci, [_vp, _ci]),
    "lmx_world_read_moved": (_ci, [_vp, _vp, _vp, _u32, C.POINTER(_u32)]),
    "lmx_world_set_bone_attachments": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "lmx_world_update_bone_attachments": (_ci, [_vp]),
    "lmx_skin_add_model": (_ci, [_vp, _u32, _vp, _vp, _i32, C.POINTER(_u32)]),
    "lmx_skin_add_mesh": (_ci, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "lmx_skin_set_instances": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_skin_upload_poses": (_ci, [_vp, _vp, _vp, _sz]),
    "lmx_skin_upload_poses_device": (_ci, [_vp, _vp, _vp, _sz]),
    "lmx_skin_set_pose_source_device": (_ci, [_vp, _vp, _vp, _sz]),
    "lmx_skin_blend_poses": (_ci, [_vp, _vp, _vp, _sz, _f32]),
    "lmx_skin_blend_poses_device": (_ci, [_vp, _vp, _vp, _sz, _f32]),
    "lmx_skin_set_mode": (_ci, [_vp, _ci]),
    "lmx_skin_set_option": (_ci, [_vp, _ci, _ci]),
    "lmx_skin_run": (_ci, [_vp]),
    "lmx_skin_read_vertices": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_skin_read_vertices_range": (_ci, [_vp, _u32, _u32, _vp, C.c_size_t]),
    "lmx_skin_device_output": (_ci, [_vp, _vp, _vp]),
    "lmx_skin_read_palette": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_skin_set_pose_writeback": (_ci, [_vp, _ci]),
    "lmx_skin_enable_dual_quats": (_ci, [_vp, _ci]),
    "lmx_skin_read_dual_quats": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_skin_read_pose": (_ci, [_vp, _u32, _vp, _vp, _u32]),
    "lmx_anim_add": (_ci, [_vp, _vp, C.POINTER(_u32)]),
    "lmx_anim_set_model_pose": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_anim_set_animables": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_anim_set_weight": (_ci, [_vp, _f32]),
    "lmx_anim_update": (_ci, [_vp, _f32]),
    "lmx_anim_eval_blend_stacks": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_anim_eval_blend_instrs": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_anim_decode_blend_stack": (_ci, [_vp, C.c_uint64, _vp, _u32, _vp, _u32, C.c_float, _vp, _u32, _vp]),
    "lmx_anim_read_times": (_ci, [_vp, _vp, _u32]),
    "lmx_anim_read_pose": (_ci, [_vp, _u32, _vp, _vp, _u32]),
    "lmx_anim_controller_check": (_ci, [_vp, C.c_uint64, _vp, _vp, _u32, _vp, _u32]),
    "lmx_anim_controller_add": (_ci, [_vp, _vp, C.c_uint64, C.POINTER(_u32)]),
    "lmx_anim_controller_input_types": (_ci, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_anim_controller_set_slots": (_ci, [_vp, _u32, _u32, _vp, _u32]),
    "lmx_anim_set_root_motion": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_animators_set": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _u32]),
    "lmx_animators_set_inputs": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_animators_set_inputs_device": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_animators_update": (_ci, [_vp, _f32]),
    "lmx_animators_read_root_motion": (_ci, [_vp, _vp, _u32]),
    "lmx_animators_device_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_animators_apply_root_motion": (_ci, [_vp]),
    "lmx_animators_read_state": (_ci, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_animators_read_instrs": (_ci, [_vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_keys_set_models": (_ci, [_vp, _vp, _u32, _vp, _u32]),
    "lmx_keys_set_instances": (_ci, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "lmx_keys_set_decals": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "lmx_keys_set_positions": (_ci, [_vp, _vp, _u32]),
    "lmx_keys_bind_world": (_ci, [_vp, _ci]),
    "lmx_keys_set_option": (_ci, [_vp, _ci, _ci]),
    "lmx_keys_run": (_ci, [_vp, _u32, _u32, _vp, _u32]),
    "lmx_keys_sort": (_ci, [_vp]),
    "lmx_keys_counts": (_ci, [_vp, _vp]),
    "lmx_keys_read_pairs": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_keys_read_instancer": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_keys_read_poses": (_ci, [_vp, _vp, _u32]),
    "lmx_keys_read_dirty": (_ci, [_vp, _vp, _u32]),
    "lmx_keys_read_state": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_keys_device_pairs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_draw_set_meshes": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_set_material_indices": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_set_transforms": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_bind_world": (_ci, [_vp, _ci]),
    "lmx_draw_set_prev_transforms": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_set_bones": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_draw_set_decals": (_ci, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmx_draw_run": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_run_pairs": (_ci, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _u32]),
    "lmx_draw_counts": (_ci, [_vp, _vp]),
    "lmx_draw_read_runs": (_ci, [_vp, _vp, _u32]),
    "lmx_draw_read_instance_data": (_ci, [_vp, _vp, _sz]),
    "lmx_draw_read_group_data": (_ci, [_vp, _vp, _sz]),
    "lmx_draw_device_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_poses_set_instances": (_ci, [_vp, _u32, _vp]),
    "lmx_poses_begin_frame": (_ci, [_vp, _u32, _u32]),
    "lmx_poses_run": (_ci, [_vp]),
    "lmx_poses_run_list": (_ci, [_vp, _vp, _u32]),
    "lmx_poses_counts": (_ci, [_vp, _vp]),
    "lmx_poses_read_slices": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_poses_read_buffer": (_ci, [_vp, _vp, _sz]),
    "lmx_poses_device_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_clusters_planes": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_clusters_set_lights": (_ci, [_vp, _u32, _vp]),
    "lmx_clusters_set_atlas": (_ci, [_vp, _u32, _vp]),
    "lmx_clusters_set_probes": (_ci, [_vp, _u32, _vp, _vp, _u32, _vp, _vp]),
    "lmx_clusters_reserve": (_ci, [_vp, _u32, _u32]),
    "lmx_clusters_run": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_clusters_run_list": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_clusters_counts": (_ci, [_vp, _vp]),
    "lmx_clusters_read_lights": (_ci, [_vp, _vp, _u32]),
    "lmx_clusters_read_light_entities": (_ci, [_vp, _vp, _u32]),
    "lmx_clusters_read_clusters": (_ci, [_vp, _vp, _u32, _vp]),
    "lmx_clusters_read_map": (_ci, [_vp, _vp, _u32]),
    "lmx_clusters_read_probes": (_ci, [_vp, _vp, _u32, _vp, _u32]),
    "lmx_clusters_device_outputs": (_ci, [_vp, _vp]),
    "lmx_rays_add_mesh": (_ci, [_vp, _u32, _vp, _vp, _vp, _u32, _u32, C.POINTER(_u32)]),
    "lmx_rays_clear_meshes": (_ci, [_vp]),
    "lmx_rays_set_models": (_ci, [_vp, _u32, _vp]),
    "lmx_rays_set_instances": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_rays_reserve": (_ci, [_vp, _u32, _u32]),
    "lmx_rays_cast": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_cast_device": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_counts": (_ci, [_vp, _vp]),
    "lmx_rays_read_hits": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_read_candidates": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_device_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_rays_set_instanced_models": (_ci, [_vp, _vp, _u32, _vp, _vp]),
    "lmx_rays_read_im_hits": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_im_counts": (_ci, [_vp, _vp]),
    "lmx_rays_device_im_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_rays_set_procedural_geometries": (_ci, [_vp, _u32, _vp]),
    "lmx_rays_set_terrains": (_ci, [_vp, _u32, _vp]),
    "lmx_rays_read_pg_hits": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_read_terrain_hits": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_read_scene_hits": (_ci, [_vp, _vp, _u32]),
    "lmx_rays_scene_counts": (_ci, [_vp, _vp]),
    "lmx_rays_device_scene_outputs": (_ci, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_viewport_frustum": (_ci, [_vp, _vp]),
    "lmx_frustum_perspective": (_ci, [_vp, _vp, _vp, _f32, _f32, _f32, _f32, _vp]),
    "lmx_frustum_ortho": (_ci, [_vp, _vp, _vp, _f32, _f32, _f32, _f32, _vp]),
    "lmx_world_blob_info": (_ci, [_vp, _sz, _vp]),
    "lmx_world_blob_read": (_ci, [_vp, _sz, _u32, _vp, _vp, _vp, _vp]),
    "lmx_world_blob_find_module": (_ci, [_vp, _sz, C.c_char_p, C.POINTER(_u32), C.POINTER(_i32)]),
    "lmx_render_blob_info": (_ci, [_vp, _sz, _vp]),
    "lmx_render_blob_read_bone_attachments": (_ci, [_vp, _sz, _u32, _vp]),
    "lmx_render_blob_read_model_instances": (_ci, [_vp, _sz, _u32, _vp, _vp, _vp, _u32]),
    "lmx_render_blob_read_instanced_models": (_ci, [_vp, _sz, _u32, _vp, _u32, _vp, _u32, _vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "lmx_im_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_im_destroy": (None, [_vp]),
    "lmx_im_set_model": (_ci, [_vp, _u32, _vp, _vp, _f32, _u32, _vp]),
    "lmx_im_set_instances": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_im_set_origins": (_ci, [_vp, _u32, _vp]),
    "lmx_im_run": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_im_read_grid": (_ci, [_vp, _u32, _vp]),
    "lmx_im_read_instances": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_im_counts": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_im_read_records": (_ci, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_im_read_indirect": (_ci, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_im_device_outputs": (_ci, [_vp, _u32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "lmx_particles_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_particles_destroy": (None, [_vp]),
    "lmx_particles_add_system": (_ci, [_vp, _u32, _u32, C.POINTER(_u32)]),
    "lmx_particles_set_program": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_particles_set_globals": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_particles_set_entity_positions": (_ci, [_vp, _u32, _vp]),
    "lmx_particles_reserve": (_ci, [_vp, _u32, _u32, _u32]),
    "lmx_particles_reset": (_ci, [_vp, _u32]),
    "lmx_particles_set_seed": (_ci, [_vp, _u32]),
    "lmx_particles_step": (_ci, [_vp, _f32]),
    "lmx_particles_fill": (_ci, [_vp]),
    "lmx_particles_counts": (_ci, [_vp, _vp, _u32]),
    "lmx_particles_read_channels": (_ci, [_vp, _u32, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_particles_read_slices": (_ci, [_vp, _vp, _u32, _vp, _u32]),
    "lmx_particles_device_outputs": (_ci, [_vp, _vp]),
    "lmx_particles_set_emitter_options": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_particles_emit_ribbons": (_ci, [_vp, _u32, _u32, _u32]),
    "lmx_particles_kill_ribbon": (_ci, [_vp, _u32, _u32, _u32]),
    "lmx_particles_apply_transforms": (_ci, [_vp, _u32, _vp]),
    "lmx_particles_ribbons": (_ci, [_vp, _u32, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_particles_add_mesh": (_ci, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "lmx_particles_clear_meshes": (_ci, [_vp]),
    "lmx_particles_set_mesh_source": (_ci, [_vp, _u32, _vp]),
    "lmx_particles_set_spline": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_grass_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_grass_destroy": (None, [_vp]),
    "lmx_grass_set_terrains": (_ci, [_vp, _u32, _vp]),
    "lmx_grass_invalidate": (_ci, [_vp, _u32]),
    "lmx_grass_set_positions": (_ci, [_vp, _u32, _vp]),
    "lmx_grass_reserve": (_ci, [_vp, _u32]),
    "lmx_grass_update": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_grass_cull": (_ci, [_vp, _u32, _vp]),
    "lmx_grass_read_quads": (_ci, [_vp, _vp, _u32, C.POINTER(_u32)]),
    "lmx_grass_read_instances": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_grass_read_draws": (_ci, [_vp, _u32, _vp, _u32, C.POINTER(_u32)]),
    "lmx_grass_counts": (_ci, [_vp, _vp, _u32]),
    "lmx_grass_write_instances": (_ci, [_vp, _u32, _vp, _u32]),
    "lmx_grass_device_outputs": (_ci, [_vp, _vp]),
    "lmx_voxels_grid": (_ci, [_vp, _vp, _u32, _vp]),
    "lmx_voxels_rng_skip": (_ci, [_u32, _u32, C.c_uint64, C.POINTER(_u32), C.POINTER(_u32)]),
    "lmx_voxels_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_voxels_destroy": (None, [_vp]),
    "lmx_voxels_set": (_ci, [_vp, _vp]),
    "lmx_voxels_begin_raster": (_ci, [_vp, _vp, _vp, _u32]),
    "lmx_voxels_raster": (_ci, [_vp, _vp, _u32, _u32, _vp, _u32, _u32]),
    "lmx_voxels_voxelize": (_ci, [_vp, _vp, _u32, _u32]),
    "lmx_voxels_compute_ao": (_ci, [_vp, _u32, _u32, _u32]),
    "lmx_voxels_rng_state": (_ci, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "lmx_voxels_blur_ao": (_ci, [_vp]),
    "lmx_voxels_set_option": (_ci, [_vp, _ci, _ci]),
    "lmx_voxels_sample": (_ci, [_vp, _vp, _u32, _vp, _vp]),
    "lmx_voxels_sample_ao": (_ci, [_vp, _vp, _u32, _vp, _vp]),
    "lmx_voxels_bake_vertex_ao": (_ci, [_vp, _vp, _u32, _u32, _f32, _vp]),
    "lmx_voxels_info": (_ci, [_vp, _vp]),
    "lmx_voxels_read": (_ci, [_vp, _vp, _u32]),
    "lmx_voxels_read_ao": (_ci, [_vp, _vp, _u32]),
    "lmx_voxels_device_outputs": (_ci, [_vp, _vp]),
    "lmx_probes_batch_bytes": (_ci, [_u32, _u32, C.POINTER(C.c_uint64)]),
    "lmx_probes_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_probes_destroy": (None, [_vp]),
    "lmx_probes_set_cubemaps": (_ci, [_vp, _u32, _u32, _vp]),
    "lmx_probes_sh_run": (_ci, [_vp]),
    "lmx_probes_mips_run": (_ci, [_vp]),
    "lmx_probes_read_sh": (_ci, [_vp, _vp, _u32]),
    "lmx_probes_read_mips": (_ci, [_vp, _vp, C.c_uint64]),
    "lmx_probes_device_outputs": (_ci, [_vp, _vp]),
    "lmx_probes_ggx_samples": (_ci, [_u32, _vp]),
    "lmx_probes_filter_run": (_ci, [_vp]),
    "lmx_probes_sample": (_ci, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "lmx_probes_read_filtered": (_ci, [_vp, _vp, C.c_uint64]),
    "lmx_probes_read_rgbm": (_ci, [_vp, _vp, C.c_uint64]),
    "lmx_texcomp_output_bytes": (_ci, [_u32, _vp, _ci, C.POINTER(C.c_uint64)]),
    "lmx_texcomp_blocks_per_round": (_u32, []),
    "lmx_texcomp_tables": (_ci, [_vp, C.c_uint64]),
    "lmx_texcomp_hist_index": (_ci, [_u32, _vp, C.POINTER(_u32)]),
    "lmx_texcomp_encode_host": (_ci, [_ci, _u32, _vp, _vp, _vp]),
    "lmx_texcomp_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_texcomp_destroy": (None, [_vp]),
    "lmx_texcomp_set_images": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_texcomp_set_images_device": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_texcomp_set_from_probes": (_ci, [_vp, _vp]),
    "lmx_texcomp_run": (_ci, [_vp, _ci]),
    "lmx_texcomp_read": (_ci, [_vp, _vp, C.c_uint64]),
    "lmx_texcomp_device_outputs": (_ci, [_vp, _vp]),
    "lmx_texcomp_chain_levels": (_u32, [_u32, _u32]),
    "lmx_texcomp_chain_bytes": (_ci, [_u32, _u32, _u32, C.POINTER(C.c_uint64)]),
    "lmx_texcomp_set_chains": (_ci, [_vp, _u32, _u32, _u32, _vp]),
    "lmx_texcomp_set_chains_device": (_ci, [_vp, _u32, _u32, _u32, _vp]),
    "lmx_texcomp_generate_mips": (_ci, [_vp, _vp]),
    "lmx_texcomp_read_pixels": (_ci, [_vp, _vp, C.c_uint64]),
    "lmx_texmips_coeffs": (_ci, [_u32, _u32, _vp, _u32]),
    "lmx_texmips_host": (_ci, [_vp, _u32, _u32, _u32, _vp, _vp]),
    "lmx_animcomp_create": (_ci, [_vp, C.POINTER(_vp)]),
    "lmx_animcomp_destroy": (None, [_vp]),
    "lmx_animcomp_set_clips": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_animcomp_set_clips_device": (_ci, [_vp, _u32, _vp, _vp]),
    "lmx_animcomp_run": (_ci, [_vp]),
    "lmx_animcomp_clip_info": (_ci, [_vp, _u32, _vp]),
    "lmx_animcomp_read_clip": (_ci, [_vp, _u32, _vp]),
    "lmx_animcomp_device_outputs": (_ci, [_vp, _vp, _vp, _vp, _vp]),
    "lmx_animcomp_compress_host": (_ci, [_vp, _vp, _vp, _vp]),
    "lmx_anim_add_compressed": (_ci, [_vp, _vp, _u32, _u32, C.POINTER(_u32)]),
    "lmx_version": (C.c_char_p, []),
}

ERROR_NAMES = {1: "INVALID_ARGUMENT", 2: "NO_DEVICE", 3: "HIP", 4: "OUT_OF_MEMORY", 5: "CAPACITY", 6: "NOT_BUILT", 7: "BUSY", 8: "INVALID", 9: "UNSUPPORTED"}
ERR_BUSY = 7


class LumixError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"LMX_ERR_{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


_lib = None


def load_library() -> C.CDLL:
    """Loads liblumix_mi355.so and declares every exported entry point. Raises if the HIP extension is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m lumixengine_amd.build` (there is no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64x3(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3))


def _f32x3(v) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(3))


class Context:
    """One GPU + one HIP stream (lmx_ctx_*)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.lmx_ctx_create(device, C.byref(h))
        if rc != 0:
            raise LumixError(rc, self.lib.lmx_last_error(None).decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.lmx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc != 0:
            raise LumixError(rc, self.lib.lmx_last_error(self.h).decode())

    def set_stream(self, hip_stream: Optional[int]):
        self.check(self.lib.lmx_ctx_set_stream(self.h, hip_stream))

    def synchronize(self):
        self.check(self.lib.lmx_ctx_synchronize(self.h))

    def profile_enable(self, on: bool = True):
        self.check(self.lib.lmx_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(self.lib.lmx_profile_reset(self.h))

    def profile_get(self, kernel: int):
        ms, n = C.c_double(0), C.c_uint64(0)
        self.check(self.lib.lmx_profile_get(self.h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class _ContextObject:
    """An object beside the context: lmx_<UNIT>_create(ctx, &h) at construction, lmx_<UNIT>_destroy(h) at close() or collection."""

    UNIT = ""  # the subclass's part of the two names

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx.check(getattr(self.lib, f"lmx_{self.UNIT}_create")(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):  # (the destroy reads its context: behind Context.close() there is nothing left to call it on)
                getattr(self.lib, f"lmx_{self.UNIT}_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- frusta (host mirror of core/geometry.cpp) ----------------------------------------------------------------
def viewport_frustum(is_ortho=False, fov=float(np.deg2rad(60.0)), ortho_size=100.0, w=1920, h=1080, pos=(0, 0, 0), rot=(0, 0, 0, 1), near=0.1,
                     far=10000.0) -> np.ndarray:
    """Viewport::getFrustum() (core/geometry.cpp:793-818)."""
    lib = load_library()
    vp = np.zeros(1, VIEWPORT)
    vp["is_ortho"], vp["fov"], vp["ortho_size"], vp["w"], vp["h"] = int(is_ortho), fov, ortho_size, w, h
    vp["pos"], vp["rot"], vp["near_plane"], vp["far_plane"] = pos, rot, near, far
    out = np.zeros(1, SHIFTED_FRUSTUM)
    rc = lib.lmx_viewport_frustum(_ptr(vp), _ptr(out))
    if rc:
        raise LumixError(rc, "lmx_viewport_frustum")
    return out


def frustum_perspective(pos, direction, up, fov, ratio, near, far) -> np.ndarray:
    out = np.zeros(1, SHIFTED_FRUSTUM)
    rc = load_library().lmx_frustum_perspective(_ptr(_f64x3(pos)), _ptr(_f32x3(direction)), _ptr(_f32x3(up)), fov, ratio, near, far, _ptr(out))
    if rc:
        raise LumixError(rc, "lmx_frustum_perspective")
    return out


def frustum_ortho(pos, direction, up, width, height, near, far) -> np.ndarray:
    out = np.zeros(1, SHIFTED_FRUSTUM)
    rc = load_library().lmx_frustum_ortho(_ptr(_f64x3(pos)), _ptr(_f32x3(direction)), _ptr(_f32x3(up)), width, height, near, far, _ptr(out))
    if rc:
        raise LumixError(rc, "lmx_frustum_ortho")
    return out


def transform_compose(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Transform::compose (core/math.cpp:801-807), element-wise over two TRANSFORM arrays."""
    lib = load_library()
    a, b = np.ascontiguousarray(a, TRANSFORM), np.ascontiguousarray(b, TRANSFORM)
    out = np.zeros(len(a), TRANSFORM)
    for i in range(len(a)):
        lib.lmx_transform_compose(_ptr(a[i : i + 1]), _ptr(b[i : i + 1]), _ptr(out[i : i + 1]))
    return out


def transform_compute_local(parent: np.ndarray, child: np.ndarray) -> np.ndarray:
    """Transform::computeLocal (core/math.cpp:809-816)."""
    lib = load_library()
    parent, child = np.ascontiguousarray(parent, TRANSFORM), np.ascontiguousarray(child, TRANSFORM)
    out = np.zeros(len(parent), TRANSFORM)
    for i in range(len(parent)):
        lib.lmx_transform_compute_local(_ptr(parent[i : i + 1]), _ptr(child[i : i + 1]), _ptr(out[i : i + 1]))
    return out


class CullResult:
    """Result of one cull call: the visible ids per (frustum, type), resident in HBM (view slot) until the slot is reused.

    The reference returns a linked list of 4 KiB pages, each tagged with a renderable type (culling_system.h:17-56);
    `ids(frustum, type)` is the concatenation of the pages of that type, `pages(...)` re-creates the page split.
    """

    def __init__(self, cs: "CullingSystem", view: int, n_frusta: int):
        self.cs, self.view, self.n_frusta = cs, view, n_frusta
        self._counts = None

    def counts(self) -> np.ndarray:
        if self._counts is None:
            out = np.zeros((self.n_frusta, MAX_TYPES), np.uint32)
            self.cs.ctx.check(self.cs.lib.lmx_cull_counts(self.cs.ctx.h, self.view, _ptr(out)))
            self._counts = out
        return self._counts

    def count(self, frustum: int = 0) -> int:
        return int(self.counts()[frustum].sum())

    def ids(self, frustum: int = 0, type_: int = 0) -> np.ndarray:
        n = int(self.counts()[frustum, type_])
        out = np.zeros(n, np.int32)
        got = C.c_uint32(0)
        self.cs.ctx.check(self.cs.lib.lmx_cull_read(self.cs.ctx.h, self.view, frustum, type_, _ptr(out), n, C.byref(got)))
        return out[: got.value]

    def all_ids(self, frustum: int = 0):
        """(ids, types) over all types, like walking the whole CullResult list (lmx_cull_read_all: two host waits)."""
        n = int(self.counts()[frustum].sum())
        out = np.zeros(max(n, 1), np.int32)
        cnt = np.zeros(MAX_TYPES, np.uint32)
        self.cs.ctx.check(self.cs.lib.lmx_cull_read_all(self.cs.ctx.h, self.view, frustum, _ptr(out), len(out), _ptr(cnt)))
        return out[: int(cnt.sum())], np.repeat(np.arange(MAX_TYPES, dtype=np.uint8), cnt)

    def map_all(self, frustum: int = 0):
        """(ids, types) like all_ids, through lmx_cull_map_all (normally one host wait; the ids are copied out of the library's pinned
        buffer here - a C caller reads them in place)."""
        p = C.POINTER(C.c_int32)()
        cnt = np.zeros(MAX_TYPES, np.uint32)
        self.cs.ctx.check(self.cs.lib.lmx_cull_map_all(self.cs.ctx.h, self.view, frustum, C.byref(p), _ptr(cnt)))
        n = int(cnt.sum())
        ids = np.frombuffer(C.string_at(p, 4 * n), np.int32) if n else np.zeros(0, np.int32)
        return ids, np.repeat(np.arange(MAX_TYPES, dtype=np.uint8), cnt)

    def pages(self, frustum: int = 0, type_: int = 0, page_ids: int = 1020):
        a = self.ids(frustum, type_)
        return [a[i : i + page_ids] for i in range(0, len(a), page_ids)]

    def device_result(self, frustum: int = 0):
        """(d_ids ptr, d_counts ptr, type_offsets[MAX_TYPES], capacity) for GPU-side consumers."""
        d_ids, d_counts, cap = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        offs = np.zeros(MAX_TYPES, np.uint32)
        self.cs.ctx.check(self.cs.lib.lmx_cull_device_result(self.cs.ctx.h, self.view, frustum, C.byref(d_ids), C.byref(d_counts), _ptr(offs), C.byref(cap)))
        return d_ids.value, d_counts.value, offs, cap.value


class CullingSystem:
    """GPU-backed CullingSystem (src/renderer/culling_system.h:58-77)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib

    # bulk form of `add` for scene load
    def build(self, entity, type_, pos, radius):
        entity = np.ascontiguousarray(entity, np.int32)
        type_ = np.ascontiguousarray(type_, np.uint8)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        radius = np.ascontiguousarray(radius, np.float32)
        assert len(entity) == len(type_) == len(pos) == len(radius)
        self.ctx.check(self.lib.lmx_cull_build(self.ctx.h, len(entity), _ptr(entity), _ptr(type_), _ptr(pos), _ptr(radius)))

    def add(self, entity: int, type_: int, pos, radius: float):
        self.ctx.check(self.lib.lmx_cull_add(self.ctx.h, int(entity), int(type_), _ptr(_f64x3(pos)), float(radius)))

    def remove(self, entity: int):
        self.ctx.check(self.lib.lmx_cull_remove(self.ctx.h, int(entity)))

    def set(self, entity: int, pos, radius: float):
        self.ctx.check(self.lib.lmx_cull_set(self.ctx.h, int(entity), _ptr(_f64x3(pos)), float(radius)))

    def setPosition(self, entity: int, pos):
        self.ctx.check(self.lib.lmx_cull_set_position(self.ctx.h, int(entity), _ptr(_f64x3(pos))))

    def setRadius(self, entity: int, radius: float):
        self.ctx.check(self.lib.lmx_cull_set_radius(self.ctx.h, int(entity), float(radius)))

    def getRadius(self, entity: int) -> float:
        r = C.c_float(0)
        self.ctx.check(self.lib.lmx_cull_get_radius(self.ctx.h, int(entity), C.byref(r)))
        return r.value

    def isAdded(self, entity: int) -> bool:
        return bool(self.lib.lmx_cull_is_added(self.ctx.h, int(entity)))

    def flush(self):
        self.ctx.check(self.lib.lmx_cull_flush(self.ctx.h))

    def addMany(self, entity, type_, pos, radius):
        entity = np.ascontiguousarray(entity, np.int32)
        type_ = np.ascontiguousarray(type_, np.uint8)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        radius = np.ascontiguousarray(radius, np.float32)
        assert len(entity) == len(type_) == len(pos) == len(radius)
        self.ctx.check(self.lib.lmx_cull_add_many(self.ctx.h, len(entity), _ptr(entity), _ptr(type_), _ptr(pos), _ptr(radius)))

    def setMany(self, entity, pos, radius):
        entity = np.ascontiguousarray(entity, np.int32)
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        radius = np.ascontiguousarray(radius, np.float32)
        assert len(entity) == len(pos) == len(radius)
        self.ctx.check(self.lib.lmx_cull_set_many(self.ctx.h, len(entity), _ptr(entity), _ptr(pos), _ptr(radius)))

    def removeMany(self, entity):
        entity = np.ascontiguousarray(entity, np.int32)
        self.ctx.check(self.lib.lmx_cull_remove_many(self.ctx.h, len(entity), _ptr(entity)))

    def compact(self):
        self.ctx.check(self.lib.lmx_cull_compact(self.ctx.h))

    def updateStats(self):
        v = [C.c_uint32(0) for _ in range(4)]
        self.ctx.check(self.lib.lmx_cull_update_stats(self.ctx.h, *[C.byref(x) for x in v]))
        return dict(zip(("static", "bound", "overflow", "tombstones"), (x.value for x in v)))

    def asyncStats(self):
        """LMX_CULL_OPT_ASYNC_COMPACTION: {"state": -1 off / 0 idle / 1 requested / 2 running / 3 ready / 4 failed, "jobs", "swaps", "ops_replayed_at_swaps", "log_drains"}"""
        st, jobs, swaps, ops, drains = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(self.lib.lmx_cull_async_stats(self.ctx.h, C.byref(st), C.byref(jobs), C.byref(swaps), C.byref(ops), C.byref(drains)))
        return {"state": st.value, "jobs": jobs.value, "swaps": swaps.value, "ops_replayed_at_swaps": ops.value, "log_drains": drains.value}

    def setOption(self, option: int, value: int):
        self.ctx.check(self.lib.lmx_cull_set_option(self.ctx.h, int(option), int(value)))

    def stats(self):
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self.ctx.check(self.lib.lmx_cull_stats(self.ctx.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"entities": a.value, "cells": b.value, "chunks": c.value}

    def layoutInfo(self):
        """{"cell_key_bytes": 8 (keys relative to the tile's box) | 16, "table_bytes": per-tile tables + chunk headers a full cull reads}"""
        kb, tb = C.c_uint32(0), C.c_uint64(0)
        self.ctx.check(self.lib.lmx_cull_layout_info(self.ctx.h, C.byref(kb), C.byref(tb)))
        return {"cell_key_bytes": kb.value, "table_bytes": tb.value}

    def bindOutput(self, view: int, d_ids: Optional[int], ids_capacity: int, d_counts: Optional[int]):
        """Result slot `view` writes into caller-owned device memory (raw pointers, e.g. torch tensors' data_ptr())."""
        self.ctx.check(self.lib.lmx_cull_bind_output(self.ctx.h, view, d_ids, ids_capacity, d_counts))

    def setPassWidth(self, frusta_per_pass: int):
        self.ctx.check(self.lib.lmx_cull_set_pass_width(self.ctx.h, frusta_per_pass))

    def packDevice(self, view: int = 0, frustum: int = 0):
        """(device pointer, words) of the packed record [8 counts | ids, types back to back] of the view's last cull - no host wait."""
        p, n = C.c_void_p(), _u32(0)
        self.ctx.check(self.lib.lmx_cull_pack_device(self.ctx.h, view, frustum, C.byref(p), C.byref(n)))
        return p.value, n.value

    def cull(self, frusta: np.ndarray, type_: int = TYPE_ALL, view: int = 0) -> CullResult:
        """cull(frustum[, type]); `frusta` may hold up to 8 ShiftedFrustum records tested in one pass."""
        frusta = np.ascontiguousarray(frusta, SHIFTED_FRUSTUM).reshape(-1)
        self.ctx.check(self.lib.lmx_cull(self.ctx.h, view, _ptr(frusta), len(frusta), type_))
        return CullResult(self, view, len(frusta))


def exchange_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0): 128 opaque bytes every rank passes to VisibleExchange."""
    buf = np.zeros(128, np.uint8)
    rc = load_library().lmx_exchange_unique_id(_ptr(buf))
    if rc:
        raise LumixError(rc, "lmx_exchange_unique_id (is RCCL installed?)")
    return buf.tobytes()


class ExchangeStats(C.Structure):
    """LmxExchangeStats (include/lumix_mi355.h)"""
    _fields_ = [("n_frusta", C.c_uint32), ("record_words", C.c_uint32), ("caps", C.c_uint32 * 8), ("max_visible", C.c_uint32 * 8), ("overflow_mask", C.c_uint32),
                ("used_words_own", C.c_uint32), ("used_words_max", C.c_uint32), ("mode", C.c_int32), ("bytes_shipped_per_peer", C.c_uint64), ("bytes_used", C.c_uint64),
                ("gather_us", C.c_double), ("gather_us_record_words", C.c_uint32), ("reserved", C.c_uint32)]


class VisibleExchange:
    """lmx_exchange_*: per frame one cull of this rank's entities + one RCCL all-gather of [8 counts | cap ids] per rank."""

    def __init__(self, ctx: Context, rank: int, world: int, unique_id: bytes, ids_per_rank: int):
        self.ctx, self.lib, self.rank, self.world, self.cap = ctx, ctx.lib, rank, world, int(ids_per_rank)
        uid = np.frombuffer(unique_id, np.uint8).copy()
        h = C.c_void_p()
        ctx.check(self.lib.lmx_exchange_create(ctx.h, rank, world, _ptr(uid), self.cap, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lmx_exchange_destroy(self.h)
            self.h = None

    def cull(self, frustum: np.ndarray, type_: int = TYPE_ALL) -> int:
        frustum = np.ascontiguousarray(frustum, SHIFTED_FRUSTUM).reshape(-1)
        slot = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_exchange_cull(self.h, _ptr(frustum), type_, C.byref(slot)))
        self.last_slot = slot.value
        return slot.value

    def cullMany(self, frusta: np.ndarray, type_: int = TYPE_ALL) -> int:
        """The frame's views (<= 8 frusta, the same number on every rank) in one pass + ONE all-gather; returns the slot."""
        frusta = np.ascontiguousarray(frusta, SHIFTED_FRUSTUM).reshape(-1)
        slot = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_exchange_cull_many(self.h, _ptr(frusta), len(frusta), type_, C.byref(slot)))
        self.last_slot = slot.value
        return slot.value

    def layout(self, slot: int) -> dict:
        """lmx_exchange_layout: {"n_frusta", "caps"[n], "offsets"[n] (words from a rank's record start), "record_words"} of the slot's last frame"""
        n, rec = C.c_uint32(0), C.c_uint32(0)
        caps, offs = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
        self.ctx.check(self.lib.lmx_exchange_layout(self.h, slot, C.byref(n), _ptr(caps), _ptr(offs), C.byref(rec)))
        return {"n_frusta": n.value, "caps": [int(c) for c in caps[: n.value]], "offsets": [int(o) for o in offs[: n.value]], "record_words": rec.value}

    def readMany(self, slot: int, rank: int, frustum: int):
        """(counts[8], ids) of one (rank, frustum) sub-record; ids clipped to the sub-record's capacity (layout(slot)["caps"][frustum])."""
        cap_f = self.layout(slot)["caps"][frustum]
        counts = np.zeros(MAX_TYPES, np.uint32)
        ids = np.zeros(max(cap_f, 1), np.int32)
        self.ctx.check(self.lib.lmx_exchange_read_many(self.h, slot, rank, frustum, _ptr(counts), _ptr(ids), cap_f))
        return counts, ids[: min(int(counts.sum()), cap_f)]

    def setCaps(self, caps, keep_fixed: bool = False):
        """capacities of the sub-records of frames of len(caps) frusta from now on (every rank: the same call at the same point)"""
        caps = np.ascontiguousarray(caps, np.uint32)
        self.ctx.check(self.lib.lmx_exchange_set_caps(self.h, len(caps), _ptr(caps), 1 if keep_fixed else 0))

    def timeGather(self, n_frusta: int = 1):
        """COLLECTIVE: (us per all-gather of the record a frame of n_frusta frusta ships now, that record's words per rank)"""
        us, words = C.c_double(-1.0), C.c_uint32(0)
        self.ctx.check(self.lib.lmx_exchange_time_gather(self.h, n_frusta, C.byref(us), C.byref(words)))
        return us.value, words.value

    def stats(self, slot: int) -> dict:
        """lmx_exchange_stats of the slot's last frame (waits for its gather)"""
        st = ExchangeStats()
        self.ctx.check(self.lib.lmx_exchange_stats(self.h, slot, C.byref(st)))
        n = st.n_frusta
        return {"n_frusta": n, "record_words": st.record_words, "caps": list(st.caps[:n]), "max_visible": list(st.max_visible[:n]), "overflow_mask": st.overflow_mask,
                "used_words_own": st.used_words_own, "used_words_max": st.used_words_max, "mode": ("inline", "side", "p2p")[st.mode],
                "bytes_shipped_per_peer": int(st.bytes_shipped_per_peer), "bytes_used": int(st.bytes_used),
                "gather_us": st.gather_us if st.gather_us >= 0 else None, "gather_us_record_words": st.gather_us_record_words}

    def wait(self, slot: int):
        self.ctx.check(self.lib.lmx_exchange_wait(self.h, slot))

    def info(self) -> dict:
        """how frames of the shape that ran last run: {"mode": "inline" | "side" | "p2p", "gather_us": one all-gather of that shape's record as last timed (None: never), "why"}"""
        mode, us, why = C.c_int(0), C.c_double(-1.0), C.c_char_p()
        self.ctx.check(self.lib.lmx_exchange_info(self.h, C.byref(mode), C.byref(us), C.byref(why)))
        return {"mode": ("inline", "side", "p2p")[mode.value], "gather_us": us.value if us.value >= 0 else None, "why": (why.value or b"").decode()}

    def read(self, slot: int, rank: int):
        """(counts[8], ids) of one rank's gathered record of a one-frustum frame (ids of type 0 first; clipped to the record's capacity)."""
        return self.readMany(slot, rank, 0)


WORLD_INFO = np.dtype([("n", "<u4"), ("n_live", "<u4"), ("n_levels", "<u4"), ("fused", "<u4"), ("edits", "<u4"), ("reserved", "<u4", 3)])  # LmxWorldInfo


class World:
    """Batch form of World's transform hierarchy (src/engine/world.cpp:255-282)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n = 0

    def build(self, parent, transforms):
        parent = np.ascontiguousarray(parent, np.int32)
        transforms = np.ascontiguousarray(transforms, TRANSFORM)
        assert len(parent) == len(transforms)
        self.n = len(parent)
        self.ctx.check(self.lib.lmx_world_build(self.ctx.h, self.n, _ptr(parent), _ptr(transforms)))

    def buildWithWorld(self, parent, local_transforms, world_transforms):
        """Mirror of a live World: the stored world transform of every entity + Hierarchy::local_transform of the parented ones."""
        parent = np.ascontiguousarray(parent, np.int32)
        local_transforms = np.ascontiguousarray(local_transforms, TRANSFORM)
        world_transforms = np.ascontiguousarray(world_transforms, TRANSFORM)
        assert len(parent) == len(local_transforms) == len(world_transforms)
        self.n = len(parent)
        self.ctx.check(self.lib.lmx_world_build_with_world(self.ctx.h, self.n, _ptr(parent), _ptr(local_transforms), _ptr(world_transforms)))

    def setTransforms(self, entity, transforms):
        """World::setTransform for roots / World::setLocalTransform for children, staged until propagate()."""
        entity = np.ascontiguousarray(entity, np.int32)
        transforms = np.ascontiguousarray(transforms, TRANSFORM)
        assert len(entity) == len(transforms)
        self.ctx.check(self.lib.lmx_world_set_transforms(self.ctx.h, len(entity), _ptr(entity), _ptr(transforms)))

    def setWorldTransforms(self, entity, transforms):
        """World::setTransform (world-space) on any entity, staged until propagate()."""
        entity = np.ascontiguousarray(entity, np.int32)
        transforms = np.ascontiguousarray(transforms, TRANSFORM)
        assert len(entity) == len(transforms)
        self.ctx.check(self.lib.lmx_world_set_world_transforms(self.ctx.h, len(entity), _ptr(entity), _ptr(transforms)))

    def setTransformsDevice(self, n: int, d_entity: int, d_transforms: int):
        """Same as setTransforms with both arrays already resident in HBM (raw device pointers)."""
        self.ctx.check(self.lib.lmx_world_set_transforms_device(self.ctx.h, n, d_entity, d_transforms))

    def bindCulling(self, entity, model_radius):
        entity = np.ascontiguousarray(entity, np.int32)
        model_radius = np.ascontiguousarray(model_radius, np.float32)
        self.ctx.check(self.lib.lmx_world_bind_culling(self.ctx.h, len(entity), _ptr(entity), _ptr(model_radius)))

    def setParent(self, new_parent: int, child: int):
        """World::setParent (world.cpp:619-701); new_parent < 0 detaches."""
        self.ctx.check(self.lib.lmx_world_set_parent(self.ctx.h, int(new_parent), int(child)))

    def edit(self, destroy=(), create=(), create_transforms=None, reparent=()):
        """World::destroyEntity / createEntity / setParent for a batch (lmx_world_edit): every destroy, then every create (roots with
        `create_transforms` as world transforms), then reparent = [(new_parent, child), ...] in list order; new_parent < 0 detaches.
        The slot order is derived again on the device; a refused batch (LumixError) leaves the world as it was."""
        destroy = np.ascontiguousarray(destroy, np.int32).reshape(-1)
        create = np.ascontiguousarray(create, np.int32).reshape(-1)
        tr = np.zeros(0, TRANSFORM) if create_transforms is None else np.ascontiguousarray(create_transforms, TRANSFORM).reshape(-1)
        assert len(tr) == len(create)
        rp = np.ascontiguousarray(reparent, np.int32).reshape(-1, 2)
        new_parent, child = np.ascontiguousarray(rp[:, 0]), np.ascontiguousarray(rp[:, 1])
        self.ctx.check(self.lib.lmx_world_edit(self.ctx.h, len(destroy), _ptr(destroy) if len(destroy) else None, len(create), _ptr(create) if len(create) else None,
                                               _ptr(tr) if len(tr) else None, len(child), _ptr(new_parent) if len(child) else None, _ptr(child) if len(child) else None))
        self.n = self.info()["n"]

    def info(self) -> dict:
        """{"n": index range, "n_live", "n_levels", "fused": the next propagate() takes the one-launch path, "edits": successful edit() calls}"""
        out = np.zeros(1, WORLD_INFO)
        self.ctx.check(self.lib.lmx_world_info(self.ctx.h, _ptr(out)))
        return {k: int(out[k][0]) for k in ("n", "n_live", "n_levels", "fused", "edits")}

    def setBoneAttachments(self, entity, parent_entity, skin_instance, bone_index, relative):
        """RenderModuleImpl::m_bone_attachments: entity follows bone `bone_index` of `skin_instance`, posed on `parent_entity`."""
        a = [np.ascontiguousarray(entity, np.int32), np.ascontiguousarray(parent_entity, np.int32), np.ascontiguousarray(skin_instance, np.uint32),
             np.ascontiguousarray(bone_index, np.uint32), np.ascontiguousarray(relative, LOCAL_RIGID)]
        self.ctx.check(self.lib.lmx_world_set_bone_attachments(self.ctx.h, len(a[0]), *[_ptr(x) for x in a]))

    def updateBoneAttachments(self):
        self.ctx.check(self.lib.lmx_world_update_bone_attachments(self.ctx.h))

    def getLocalTransforms(self) -> np.ndarray:
        out = np.zeros(self.n, TRANSFORM)
        self.ctx.check(self.lib.lmx_world_read_local_transforms(self.ctx.h, _ptr(out), self.n))
        return out

    def propagate(self):
        self.ctx.check(self.lib.lmx_world_propagate(self.ctx.h))

    def getTransforms(self) -> np.ndarray:
        out = np.zeros(self.n, TRANSFORM)
        self.ctx.check(self.lib.lmx_world_read_transforms(self.ctx.h, _ptr(out), self.n))
        return out

    def setOption(self, option: int, value: int):
        """WORLD_OPT_FUSED_LEVELS: 1 = hierarchies of <= 8 levels propagate in one launch, 0 (default) = one launch per level."""
        self.ctx.check(self.lib.lmx_world_set_option(self.ctx.h, option, value))

    def trackMoved(self, on: bool = True):
        """propagate() collects the entities whose world transform changed (what World::transformEntity would have visited)."""
        self.ctx.check(self.lib.lmx_world_track_moved(self.ctx.h, int(on)))

    def readMoved(self):
        """(entity int32[k], TRANSFORM[k]) moved by the propagate() calls since the last read; an entity moved by two of them is listed twice, newest last."""
        cap = max(2 * self.n, 1)
        ent, tr, n = np.zeros(cap, np.int32), np.zeros(cap, TRANSFORM), _u32(0)
        self.ctx.check(self.lib.lmx_world_read_moved(self.ctx.h, _ptr(ent), _ptr(tr), cap, C.byref(n)))
        return ent[: n.value].copy(), tr[: n.value].copy()


WORLD_BLOB_INFO = np.dtype([(k, "<u4") for k in ("version", "flags", "n_modules", "uncompressed_size", "compressed_size", "n_entities", "max_entity_index", "n_names",
                                                  "n_hierarchy")])


def world_blob_read(data: bytes):
    """Serialized World (engine/world.cpp:837-1043) -> (info dict, parent, transforms for World.build, world transforms, valid). Host only."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    info = np.zeros(1, WORLD_BLOB_INFO)
    rc = lib.lmx_world_blob_info(_ptr(buf), len(buf), _ptr(info))
    if rc != 0:
        raise LumixError(rc, "not a current, LZ4-compressed World blob")
    n = int(info["max_entity_index"][0]) + 1 if info["n_entities"][0] else 0
    parent, tr, world, valid = np.zeros(n, np.int32), np.zeros(n, TRANSFORM), np.zeros(n, TRANSFORM), np.zeros(n, np.uint8)
    rc = lib.lmx_world_blob_read(_ptr(buf), len(buf), n, _ptr(parent), _ptr(tr), _ptr(world), _ptr(valid))
    if rc != 0:
        raise LumixError(rc, "World blob truncated or inconsistent")
    return {k: int(info[k][0]) for k in WORLD_BLOB_INFO.names}, parent, tr, world, valid


RENDER_BLOB_INFO = np.dtype([(k, np.int32 if k == "version" else np.uint32) for k in (
    "version", "payload_offset", "payload_size", "n_cameras", "n_model_instance_slots", "n_model_instances", "n_point_lights", "n_environments", "n_terrains",
    "n_particle_systems", "n_bone_attachments", "n_environment_probes", "n_reflection_probes", "n_decals", "n_curve_decals", "n_instanced_models",
    "n_procedural_geometries", "model_paths_size")])
BLOB_BONE_ATTACHMENT = np.dtype([("bone_name_hash", np.uint64), ("entity", np.int32), ("parent_entity", np.int32), ("pos", np.float32, 3), ("rot", np.float32, 4), ("_pad", np.uint32)])


def world_blob_find_module(data: bytes, name: str):
    """(payload offset in the decompressed blob, serialized version) of module `name`, or None. Host only."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    off, ver = _u32(0), _i32(0)
    rc = lib.lmx_world_blob_find_module(_ptr(buf), len(buf), name.encode(), C.byref(off), C.byref(ver))
    return None if rc != 0 else (int(off.value), int(ver.value))


def render_blob_read(data: bytes):
    """The "renderer" module's payload of a serialized World (render_module.cpp:962-976): (info dict, bone attachments, {entity: model path}).
    Host only."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    info = np.zeros(1, RENDER_BLOB_INFO)
    rc = lib.lmx_render_blob_info(_ptr(buf), len(buf), _ptr(info))
    if rc != 0:
        raise LumixError(rc, "no readable renderer payload (RenderModuleVersion 16..18) in this World blob")
    att = np.zeros(int(info["n_bone_attachments"][0]), BLOB_BONE_ATTACHMENT)
    rc = lib.lmx_render_blob_read_bone_attachments(_ptr(buf), len(buf), len(att), _ptr(att) if len(att) else None)
    if rc != 0:
        raise LumixError(rc, "bone attachment records truncated")
    n = int(info["n_model_instance_slots"][0])
    flags, off = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
    paths = np.zeros(max(int(info["model_paths_size"][0]), 1), np.uint8)
    rc = lib.lmx_render_blob_read_model_instances(_ptr(buf), len(buf), n, _ptr(flags), _ptr(off), _ptr(paths), len(paths))
    if rc != 0:
        raise LumixError(rc, "model instance records truncated")
    table = paths.tobytes()
    models = {}
    for e in range(n):
        if flags[e] & 4:
            models[e] = None if off[e] == 0xFFFFFFFF else table[off[e] : table.index(b"\0", off[e])].decode()
    return {k: int(info[k][0]) for k in RENDER_BLOB_INFO.names}, att, models


IM_INSTANCE = np.dtype([("rot", "<f4", 3), ("lod", "<f4"), ("pos", "<f4", 3), ("scale", "<f4")])  # LmxImInstance = InstancedModel::InstanceData
BLOB_INSTANCED_MODEL = np.dtype([("entity", "<i4"), ("path_offset", "<u4"), ("first_instance", "<u4"), ("instance_count", "<u4")])
IM_CELL = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("from_instance", "<u4"), ("instance_count", "<u4")])
IM_GRID = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("placed", "<u4"), ("unplaced", "<u4"), ("cells", IM_CELL, 16)])
IM_VIEW = np.dtype([("camera_pos", "<f8", 3), ("lod_multiplier", "<f4"), ("time_delta", "<f4"), ("is_shadow", "<u4"), ("_pad", "<u4")])
IM_INDIRECT = np.dtype([("vertex_count", "<u4"), ("instance_count", "<u4"), ("first_index", "<u4"), ("base_vertex", "<u4"), ("base_instance", "<u4")])
IM_COUNTS = np.dtype([("bin_count", "<u4", 4), ("bin_offset", "<u4", 4), ("indirect_offset", "<u4"), ("mesh_count", "<u4"), ("instances", "<u4"), ("unplaced", "<u4")])
IM_MAX_MESHES = 31


def render_blob_read_instanced_models(data: bytes):
    """The instanced-model section of a World blob's renderer payload (render_module.cpp:702-723): [{entity, path, instances IM_INSTANCE[n]}]. Host only."""
    lib = load_library()
    buf = np.frombuffer(data, np.uint8)
    nm, ni, npath = _u32(0), _u32(0), _u32(0)
    rc = lib.lmx_render_blob_read_instanced_models(_ptr(buf), len(buf), 0, None, 0, None, 0, None, C.byref(nm), C.byref(ni), C.byref(npath))
    if rc not in (0, 5):
        raise LumixError(rc, "no readable renderer payload in this World blob")
    models = np.zeros(max(nm.value, 1), BLOB_INSTANCED_MODEL)
    inst = np.zeros(max(ni.value, 1), IM_INSTANCE)
    paths = np.zeros(max(npath.value, 1), np.uint8)
    rc = lib.lmx_render_blob_read_instanced_models(_ptr(buf), len(buf), len(models), _ptr(models), len(inst), _ptr(inst), len(paths), _ptr(paths), None, None, None)
    if rc != 0:
        raise LumixError(rc, "instanced model records truncated")
    table = paths.tobytes()
    out = []
    for m in models[: nm.value]:
        o = int(m["path_offset"])
        f, n = int(m["first_instance"]), int(m["instance_count"])
        out.append({"entity": int(m["entity"]), "path": table[o : table.index(b"\0", o)].decode(), "instances": inst[f : f + n].copy()})
    return out


def im_view(camera_pos=(0, 0, 0), lod_multiplier=1.0, time_delta=1 / 60, is_shadow=False) -> np.ndarray:
    """LmxImView: what encodeInstancedModels reads of a view (pipeline.cpp:2449-2660)."""
    v = np.zeros(1, IM_VIEW)
    v["camera_pos"], v["lod_multiplier"], v["time_delta"], v["is_shadow"] = camera_pos, lod_multiplier, time_delta, int(is_shadow)
    return v


class InstancedModels(_ContextObject):
    """InstancedModel grids + encodeInstancedModels on the device (lmx_im_*). Model ids are dense: addModel appends."""

    UNIT = "im"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.n_models = 0
        self.n = []

    def setModel(self, model: int, lod_distances, lod_indices, origin_radius: float, indices_count):
        ld = np.ascontiguousarray(lod_distances, np.float32).reshape(4)
        li = np.ascontiguousarray(np.asarray(lod_indices, np.int32).reshape(5, 2))
        ic = np.ascontiguousarray(indices_count, np.uint32)
        self.ctx.check(self.lib.lmx_im_set_model(self.h, model, _ptr(ld), _ptr(li), float(origin_radius), len(ic), _ptr(ic) if len(ic) else None))
        if model == self.n_models:
            self.n_models += 1
            self.n.append(0)

    def addModel(self, lod_distances, lod_indices, origin_radius: float, indices_count) -> int:
        self.setModel(self.n_models, lod_distances, lod_indices, origin_radius, indices_count)
        return self.n_models - 1

    def setInstances(self, model: int, instances):
        inst = np.ascontiguousarray(instances, IM_INSTANCE)
        self.ctx.check(self.lib.lmx_im_set_instances(self.h, model, len(inst), _ptr(inst) if len(inst) else None))
        if model < len(self.n):
            self.n[model] = len(inst)

    def setOrigins(self, pos_xyz):
        pos = np.ascontiguousarray(pos_xyz, np.float64).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_im_set_origins(self.h, len(pos), _ptr(pos)))

    def run(self, view, frustum: np.ndarray, view_slot: int = 0):
        view = np.ascontiguousarray(view, IM_VIEW)
        fr = np.ascontiguousarray(frustum, SHIFTED_FRUSTUM)
        self.ctx.check(self.lib.lmx_im_run(self.h, view_slot, _ptr(view), _ptr(fr)))

    def readGrid(self, model: int) -> np.ndarray:
        g = np.zeros(1, IM_GRID)
        self.ctx.check(self.lib.lmx_im_read_grid(self.h, model, _ptr(g)))
        return g[0]

    def readInstances(self, model: int) -> np.ndarray:
        out = np.zeros(max(self.n[model], 1), IM_INSTANCE)
        self.ctx.check(self.lib.lmx_im_read_instances(self.h, model, _ptr(out), len(out)))
        return out[: self.n[model]]

    def counts(self, view_slot: int = 0) -> np.ndarray:
        out = np.zeros(max(self.n_models, 1), IM_COUNTS)
        self.ctx.check(self.lib.lmx_im_counts(self.h, view_slot, _ptr(out), len(out)))
        return out[: self.n_models]

    def readRecords(self, view_slot: int = 0) -> np.ndarray:
        n = _u32(0)
        cap = max(int(self.counts(view_slot)["bin_count"].sum()), 1)
        out = np.zeros(cap, IM_INSTANCE)
        self.ctx.check(self.lib.lmx_im_read_records(self.h, view_slot, _ptr(out), cap, C.byref(n)))
        return out[: n.value]

    def readIndirect(self, view_slot: int = 0) -> np.ndarray:
        n = _u32(0)
        out = np.zeros(32 * max(self.n_models, 1), IM_INDIRECT)
        self.ctx.check(self.lib.lmx_im_read_indirect(self.h, view_slot, _ptr(out), len(out), C.byref(n)))
        return out[: n.value]

    def deviceOutputs(self, view_slot: int = 0):
        r, i, c = _vp(), _vp(), _vp()
        self.ctx.check(self.lib.lmx_im_device_outputs(self.h, view_slot, C.byref(r), C.byref(i), C.byref(c)))
        return r.value, i.value, c.value


def keys_view(camera_pos=(0, 0, 0), lod_ref_point=None, lod_multiplier=1.0, time_delta=1 / 60, frame_number=1, is_shadow=False,
              layer_to_bucket=None, bucket_depth_sorted=None) -> np.ndarray:
    """LmxKeysView: the per-view state PipelineImpl::createSortKeys reads (pipeline.cpp:3797-3832)."""
    kv = np.zeros(1, KEYS_VIEW)
    kv["camera_pos"] = camera_pos
    kv["lod_ref_point"] = camera_pos if lod_ref_point is None else lod_ref_point
    kv["lod_multiplier"], kv["time_delta"], kv["frame_number"], kv["is_shadow"] = lod_multiplier, time_delta, frame_number, int(is_shadow)
    kv["layer_to_bucket"] = 0xFF if layer_to_bucket is None else np.asarray(layer_to_bucket, np.uint8)
    if bucket_depth_sorted is not None:
        kv["bucket_depth_sorted"][0, : len(bucket_depth_sorted)] = np.asarray(bucket_depth_sorted, np.uint8)
    return kv


class SortKeys:
    """PipelineImpl::createSortKeys (renderer/pipeline.cpp:3789-3968) on the visible list a cull left on the device."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_entities = 0
        self.max_sort_key = 0

    def setModels(self, models, mesh_types):
        models = np.ascontiguousarray(models, KEYS_MODEL)
        mesh_types = np.ascontiguousarray(mesh_types, np.uint8)
        self.ctx.check(self.lib.lmx_keys_set_models(self.ctx.h, _ptr(models), len(models), _ptr(mesh_types), len(mesh_types)))

    def setInstances(self, model, material_offset, mesh_materials, lod, flags, dirty, pose_frame):
        model = np.ascontiguousarray(model, np.int32)
        arrs = [np.ascontiguousarray(material_offset, np.uint32), np.ascontiguousarray(mesh_materials, MESH_MATERIAL), np.ascontiguousarray(lod, np.float32),
                np.ascontiguousarray(flags, np.uint8), np.ascontiguousarray(dirty, np.uint8), np.ascontiguousarray(pose_frame, np.uint32)]
        self.n_entities = len(model)
        self.ctx.check(self.lib.lmx_keys_set_instances(self.ctx.h, len(model), _ptr(model), _ptr(arrs[0]), _ptr(arrs[1]), len(arrs[1]), _ptr(arrs[2]),
                                                       _ptr(arrs[3]), _ptr(arrs[4]), _ptr(arrs[5])))

    def setDecals(self, n_entities, decal_sort_key=None, decal_layer=None, curve_sort_key=None, curve_layer=None):
        a = [None if x is None else np.ascontiguousarray(x, t) for x, t in ((decal_sort_key, np.uint32), (decal_layer, np.uint8), (curve_sort_key, np.uint32),
                                                                             (curve_layer, np.uint8))]
        self.ctx.check(self.lib.lmx_keys_set_decals(self.ctx.h, n_entities, *[None if x is None else _ptr(x) for x in a]))
        self.n_entities = max(self.n_entities, n_entities)

    def setPositions(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_keys_set_positions(self.ctx.h, _ptr(xyz), len(xyz)))

    def bindWorld(self, on: bool = True):
        self.ctx.check(self.lib.lmx_keys_bind_world(self.ctx.h, int(on)))

    def setOption(self, option: int, value: int):
        self.ctx.check(self.lib.lmx_keys_set_option(self.ctx.h, int(option), int(value)))

    def run(self, kv, max_sort_key: int, view: int = 0, frustum: int = 0):
        kv = np.ascontiguousarray(kv, KEYS_VIEW)
        self.max_sort_key = int(max_sort_key)
        self.ctx.check(self.lib.lmx_keys_run(self.ctx.h, view, frustum, _ptr(kv), self.max_sort_key))

    def sort(self):
        self.ctx.check(self.lib.lmx_keys_sort(self.ctx.h))

    def counts(self) -> dict:
        c = np.zeros(1, KEYS_COUNTS)
        self.ctx.check(self.lib.lmx_keys_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in KEYS_COUNTS.names}

    def readPairs(self):
        n = self.counts()["pairs"]
        keys, values = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.ctx.check(self.lib.lmx_keys_read_pairs(self.ctx.h, _ptr(keys), _ptr(values), n))
        return keys, values

    def readInstancer(self):
        n = self.counts()["instanced"]
        offsets, values = np.zeros(self.max_sort_key + 2, np.uint32), np.zeros(n, np.uint64)
        self.ctx.check(self.lib.lmx_keys_read_instancer(self.ctx.h, _ptr(offsets), _ptr(values), n))
        return offsets, values

    def readPoses(self) -> np.ndarray:
        out = np.zeros(self.counts()["poses"], np.int32)
        self.ctx.check(self.lib.lmx_keys_read_poses(self.ctx.h, _ptr(out), len(out)))
        return out

    def readDirty(self) -> np.ndarray:
        out = np.zeros(self.counts()["dirty"], np.int32)
        self.ctx.check(self.lib.lmx_keys_read_dirty(self.ctx.h, _ptr(out), len(out)))
        return out

    def readState(self):
        lod, frame = np.zeros(self.n_entities, np.float32), np.zeros(self.n_entities, np.uint32)
        self.ctx.check(self.lib.lmx_keys_read_state(self.ctx.h, _ptr(lod), _ptr(frame), self.n_entities))
        return lod, frame


def draw_view(camera_pos=(0, 0, 0), frustum=None, bucket_depth_sorted=None) -> np.ndarray:
    """LmxDrawView: what PipelineImpl::createCommands reads of a view (pipeline.cpp:2758-2761, :2824)."""
    v = np.zeros(1, DRAW_VIEW)
    v["camera_pos"] = camera_pos
    if frustum is not None:
        v["frustum"] = np.ascontiguousarray(frustum, SHIFTED_FRUSTUM).reshape(-1)[0]
    if bucket_depth_sorted is not None:
        v["bucket_depth_sorted"][0, : len(bucket_depth_sorted)] = np.asarray(bucket_depth_sorted, np.uint8)
    return v


class DrawCommands:
    """PipelineImpl::createCommands (renderer/pipeline.cpp:2747-3320) + the instancer's "fill instance data" block (:3970-4014) on the
    sorted pairs a SortKeys run left on the device (lmx_draw_*)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib

    def setMeshes(self, mesh_lod):
        a = np.ascontiguousarray(mesh_lod, np.float32)
        self.ctx.check(self.lib.lmx_draw_set_meshes(self.ctx.h, _ptr(a), len(a)))

    def setMaterialIndices(self, material_index):
        a = np.ascontiguousarray(material_index, np.uint32)
        self.ctx.check(self.lib.lmx_draw_set_material_indices(self.ctx.h, _ptr(a), len(a)))

    def setTransforms(self, transforms):
        a = np.ascontiguousarray(transforms, TRANSFORM)
        self.ctx.check(self.lib.lmx_draw_set_transforms(self.ctx.h, _ptr(a), len(a)))

    def bindWorld(self, on: bool = True):
        self.ctx.check(self.lib.lmx_draw_bind_world(self.ctx.h, int(on)))

    def setPrevTransforms(self, transforms):
        a = np.ascontiguousarray(transforms, TRANSFORM)
        self.ctx.check(self.lib.lmx_draw_set_prev_transforms(self.ctx.h, _ptr(a), len(a)))

    def setBones(self, handle, offset):
        h, o = np.ascontiguousarray(handle, np.uint32), np.ascontiguousarray(offset, np.uint32)
        self.ctx.check(self.lib.lmx_draw_set_bones(self.ctx.h, _ptr(h), _ptr(o), len(h)))

    def setDecals(self, n_entities, half_extents=None, uv_scale=None, material_index=None, curve_half_extents=None, curve_uv_scale=None, curve_bezier=None,
                  curve_material_index=None):
        a = [None if x is None else np.ascontiguousarray(x, t) for x, t in ((half_extents, np.float32), (uv_scale, np.float32), (material_index, np.uint32),
                                                                             (curve_half_extents, np.float32), (curve_uv_scale, np.float32),
                                                                             (curve_bezier, np.float32), (curve_material_index, np.uint32))]
        self.ctx.check(self.lib.lmx_draw_set_decals(self.ctx.h, n_entities, *[None if x is None else _ptr(x) for x in a]))

    def run(self, view, n_batches: int = 1):
        view = np.ascontiguousarray(view, DRAW_VIEW)
        self.ctx.check(self.lib.lmx_draw_run(self.ctx.h, _ptr(view), n_batches))

    def runPairs(self, view, keys, values, n_batches: int = 1, group_offsets=None, group_values=None):
        """group_offsets (n_groups + 1 entries) / group_values: the instancer CSR to encode with the pairs; None: no instancer."""
        view = np.ascontiguousarray(view, DRAW_VIEW)
        k, v = np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(values, np.uint64)
        n_groups = 0 if group_offsets is None else len(group_offsets) - 1
        go = None if n_groups <= 0 else np.ascontiguousarray(group_offsets, np.uint32)
        gv = None if n_groups <= 0 else np.ascontiguousarray(group_values, np.uint64)
        self.ctx.check(self.lib.lmx_draw_run_pairs(self.ctx.h, _ptr(view), n_batches, _ptr(k) if len(k) else None, _ptr(v) if len(k) else None, len(k),
                                                   _ptr(go), _ptr(gv) if gv is not None and len(gv) else None, max(n_groups, 0)))

    def counts(self) -> dict:
        c = np.zeros(1, DRAW_COUNTS)
        self.ctx.check(self.lib.lmx_draw_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in DRAW_COUNTS.names}

    def readRuns(self) -> np.ndarray:
        n = self.counts()["runs"]
        out = np.zeros(max(n, 1), DRAW_RUN)
        self.ctx.check(self.lib.lmx_draw_read_runs(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def readInstanceData(self) -> np.ndarray:
        n = self.counts()["instance_bytes"]
        out = np.zeros(max(n, 1), np.uint8)
        self.ctx.check(self.lib.lmx_draw_read_instance_data(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def readGroupData(self) -> np.ndarray:
        n = self.counts()["group_records"] * 48
        out = np.zeros(max(n, 1), np.uint8)
        self.ctx.check(self.lib.lmx_draw_read_group_data(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def deviceOutputs(self):
        r, i, g, c = _vp(), _vp(), _vp(), _vp()
        self.ctx.check(self.lib.lmx_draw_device_outputs(self.ctx.h, C.byref(r), C.byref(i), C.byref(g), C.byref(c)))
        return r.value, i.value, g.value, c.value


class PoseProcessor:
    """PipelineImpl's PoseProcessor (renderer/pipeline.cpp:3730-3787) over the pose list a SortKeys run left on the device: dual-quaternion
    slices in the frame's buffer and pose->slice by entity, where DrawCommands reads it (lmx_poses_*)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_entities = 0

    def setInstances(self, skin_instance):
        a = np.ascontiguousarray(skin_instance, np.int32)
        self.n_entities = len(a)
        self.ctx.check(self.lib.lmx_poses_set_instances(self.ctx.h, len(a), _ptr(a)))

    def beginFrame(self, handle: int, base_offset: int = 0):
        self.ctx.check(self.lib.lmx_poses_begin_frame(self.ctx.h, int(handle), int(base_offset)))

    def run(self):
        self.ctx.check(self.lib.lmx_poses_run(self.ctx.h))

    def runList(self, entities):
        a = np.ascontiguousarray(entities, np.int32)
        self.ctx.check(self.lib.lmx_poses_run_list(self.ctx.h, _ptr(a) if len(a) else None, len(a)))

    def counts(self) -> dict:
        c = np.zeros(1, POSES_COUNTS)
        self.ctx.check(self.lib.lmx_poses_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in POSES_COUNTS.names}

    def readSlices(self):
        """(handle, offset) of every entity's pose->slice."""
        h, o = np.zeros(max(self.n_entities, 1), np.uint32), np.zeros(max(self.n_entities, 1), np.uint32)
        self.ctx.check(self.lib.lmx_poses_read_slices(self.ctx.h, _ptr(h), _ptr(o), self.n_entities))
        return h[: self.n_entities], o[: self.n_entities]

    def readBuffer(self, n_bytes: Optional[int] = None) -> np.ndarray:
        """The frame's buffer as bytes: what the frame used, or the first n_bytes (up to the reservation + POSES_GUARD_BYTES)."""
        n = self.counts()["bytes"] if n_bytes is None else int(n_bytes)
        out = np.zeros(max(n, 1), np.uint8)
        self.ctx.check(self.lib.lmx_poses_read_buffer(self.ctx.h, _ptr(out), n))
        return out[:n]

    def deviceOutputs(self):
        d, c = _vp(), _vp()
        self.ctx.check(self.lib.lmx_poses_device_outputs(self.ctx.h, C.byref(d), C.byref(c)))
        return d.value, c.value


def clusters_planes(frustum, w: int, h: int) -> np.ndarray:
    """The cluster planes of a view (renderer/pipeline.cpp:3464-3495), built on the host; LumixError(CAPACITY) above 64 x 64 clusters."""
    f = np.ascontiguousarray(frustum, SHIFTED_FRUSTUM).reshape(-1)[:1]
    out = np.zeros(1, CLUSTER_PLANES)
    rc = load_library().lmx_clusters_planes(_ptr(f), int(w), int(h), _ptr(out))
    if rc:
        raise LumixError(rc, "lmx_clusters_planes")
    return out


def cluster_view(camera_pos, frustum, w: int, h: int) -> np.ndarray:
    """LmxClusterView: what PipelineImpl::fillClusters reads of a view (cp.pos, cp.frustum, m_viewport.w / h)."""
    v = np.zeros(1, CLUSTER_VIEW)
    v["camera_pos"] = camera_pos
    v["frustum"] = np.ascontiguousarray(frustum, SHIFTED_FRUSTUM).reshape(-1)[0]
    v["viewport_w"], v["viewport_h"] = w, h
    return v


class ClusterFiller:
    """PipelineImpl::fillClusters (renderer/pipeline.cpp:3327-3684) over the LOCAL_LIGHT list a cull left on the device: light and probe
    records, `clusters` and `map` (lmx_clusters_*). Transforms come from DrawCommands.setTransforms / bindWorld."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.max_lights = self.map_capacity = 0

    def setLights(self, lights):
        a = np.ascontiguousarray(lights, POINT_LIGHT)
        self.ctx.check(self.lib.lmx_clusters_set_lights(self.ctx.h, len(a), _ptr(a) if len(a) else None))

    def setAtlas(self, atlas_idx=None):
        a = None if atlas_idx is None else np.ascontiguousarray(atlas_idx, np.uint32)
        self.ctx.check(self.lib.lmx_clusters_set_atlas(self.ctx.h, 0 if a is None else len(a), _ptr(a)))

    def setProbes(self, env=None, env_entities=None, refl=None, refl_entities=None):
        e = np.zeros(0, ENV_PROBE) if env is None else np.ascontiguousarray(env, ENV_PROBE)
        r = np.zeros(0, REFL_PROBE) if refl is None else np.ascontiguousarray(refl, REFL_PROBE)
        ee = np.ascontiguousarray(np.zeros(0) if env_entities is None else env_entities, np.int32)
        re_ = np.ascontiguousarray(np.zeros(0) if refl_entities is None else refl_entities, np.int32)
        assert len(e) == len(ee) and len(r) == len(re_)
        self.ctx.check(self.lib.lmx_clusters_set_probes(self.ctx.h, len(e), _ptr(e) if len(e) else None, _ptr(ee) if len(e) else None, len(r), _ptr(r) if len(r) else None,
                                                        _ptr(re_) if len(r) else None))

    def reserve(self, max_lights: int, map_capacity: int):
        self.ctx.check(self.lib.lmx_clusters_reserve(self.ctx.h, int(max_lights), int(map_capacity)))
        self.max_lights, self.map_capacity = int(max_lights), int(map_capacity)

    def run(self, view: np.ndarray, cull_view: int = 0, frustum: int = 0):
        v = np.ascontiguousarray(view, CLUSTER_VIEW)
        self.ctx.check(self.lib.lmx_clusters_run(self.ctx.h, cull_view, frustum, _ptr(v)))

    def runList(self, view: np.ndarray, entities):
        v = np.ascontiguousarray(view, CLUSTER_VIEW)
        a = np.ascontiguousarray(entities, np.int32)
        self.ctx.check(self.lib.lmx_clusters_run_list(self.ctx.h, _ptr(v), _ptr(a) if len(a) else None, len(a)))

    def counts(self) -> dict:
        c = np.zeros(1, CLUSTERS_COUNTS)
        self.ctx.check(self.lib.lmx_clusters_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in CLUSTERS_COUNTS.names}

    def _read(self, fn, dtype, used: int, n):
        n = used if n is None else int(n)
        out = np.zeros(max(n, 1), dtype)
        self.ctx.check(fn(self.ctx.h, _ptr(out), n))
        return out[:n]

    def readLights(self, n: Optional[int] = None) -> np.ndarray:
        """The light records the run left, or the first n (up to max_lights + the guard's 4 records)."""
        return self._read(self.lib.lmx_clusters_read_lights, CLUSTER_LIGHT, min(self.counts()["lights"], self.max_lights), n)

    def readLightEntities(self, n: Optional[int] = None) -> np.ndarray:
        return self._read(self.lib.lmx_clusters_read_light_entities, np.int32, min(self.counts()["lights"], self.max_lights), n)

    def readMap(self, n: Optional[int] = None) -> np.ndarray:
        return self._read(self.lib.lmx_clusters_read_map, np.int32, min(self.counts()["map_entries"], self.map_capacity), n)

    def readClusters(self):
        """(clusters, (size.x, size.y, size.z))"""
        size = np.zeros(3, np.uint32)
        out = np.zeros(64 * 64 * 16, CLUSTER)
        self.ctx.check(self.lib.lmx_clusters_read_clusters(self.ctx.h, _ptr(out), len(out), _ptr(size)))
        return out[: int(size.prod())].copy(), tuple(int(x) for x in size)

    def readProbes(self):
        """(environment probe records, reflection probe records), enabled ones in output order"""
        c = self.counts()
        e, r = np.zeros(max(c["env_probes"], 1), CLUSTER_ENV_PROBE), np.zeros(max(c["refl_probes"], 1), CLUSTER_REFL_PROBE)
        self.ctx.check(self.lib.lmx_clusters_read_probes(self.ctx.h, _ptr(e), len(e), _ptr(r), len(r)))
        return e[: c["env_probes"]], r[: c["refl_probes"]]

    def deviceOutputs(self) -> dict:
        out = np.zeros(1, np.dtype([(k, "<u8") for k in ("lights", "light_entities", "clusters", "map", "env_probes", "refl_probes", "counts")] + [("size", "<u4", 3), ("_pad", "<u4")]))
        self.ctx.check(self.lib.lmx_clusters_device_outputs(self.ctx.h, _ptr(out)))
        return {k: (tuple(int(x) for x in out[k][0]) if k == "size" else int(out[k][0])) for k in out.dtype.names if k != "_pad"}


def rays(origin, direction, t_max=np.inf, ignore=-1) -> np.ndarray:
    """LmxRay records from (n, 3) origins and NORMALISED directions; t_max / ignore broadcast."""
    o = np.asarray(origin, np.float64).reshape(-1, 3)
    r = np.zeros(len(o), RAY)
    r["origin"] = o
    r["dir"] = np.asarray(direction, np.float32).reshape(-1, 3)
    r["t_max"] = t_max
    r["ignore"] = ignore
    return r


class RayCaster:
    """RenderModuleImpl::castRay's model-instance loop with Model::castRay for batches of rays (lmx_rays_*). Transforms come from
    DrawCommands.setTransforms / bindWorld, poses from PoseProcessor.setInstances and the last Skinning.run."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self.max_rays = self.max_candidates = 0

    def clearMeshes(self):
        self.ctx.check(self.lib.lmx_rays_clear_meshes(self.ctx.h))

    def addMesh(self, positions, indices, skin=None) -> int:
        """indices: a uint16 or uint32 array (its dtype is the index width)"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        i = np.ascontiguousarray(indices)
        assert i.dtype in (np.uint16, np.uint32), i.dtype
        i = i.reshape(-1)
        sk = None if skin is None else np.ascontiguousarray(skin, SKIN)
        assert sk is None or len(sk) == len(p)
        out = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_rays_add_mesh(self.ctx.h, len(p), _ptr(p) if len(p) else None, _ptr(sk), _ptr(i) if len(i) else None, i.dtype.itemsize, len(i), C.byref(out)))
        return out.value

    def setModels(self, models):
        m = np.ascontiguousarray(models, RAY_MODEL)
        self.ctx.check(self.lib.lmx_rays_set_models(self.ctx.h, len(m), _ptr(m) if len(m) else None))

    def setInstances(self, model, flags):
        m = np.ascontiguousarray(model, np.int32)
        f = np.ascontiguousarray(flags, np.uint8)
        assert len(m) == len(f)
        self.ctx.check(self.lib.lmx_rays_set_instances(self.ctx.h, len(m), _ptr(m) if len(m) else None, _ptr(f) if len(m) else None))

    def reserve(self, max_rays: int, max_candidates: int):
        self.ctx.check(self.lib.lmx_rays_reserve(self.ctx.h, int(max_rays), int(max_candidates)))
        self.max_rays, self.max_candidates = int(max_rays), int(max_candidates)

    def cast(self, rays_):
        r = np.ascontiguousarray(rays_, RAY)
        self.ctx.check(self.lib.lmx_rays_cast(self.ctx.h, _ptr(r) if len(r) else None, len(r)))

    def castDevice(self, d_rays: int, n: int):
        self.ctx.check(self.lib.lmx_rays_cast_device(self.ctx.h, C.c_void_p(d_rays), int(n)))

    def counts(self) -> dict:
        c = np.zeros(1, RAYS_COUNTS)
        self.ctx.check(self.lib.lmx_rays_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in RAYS_COUNTS.names}

    def readHits(self) -> np.ndarray:
        n = self.counts()["rays"]
        out = np.zeros(max(n, 1), RAY_HIT)
        self.ctx.check(self.lib.lmx_rays_read_hits(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def readCandidates(self, n: Optional[int] = None) -> np.ndarray:
        """The candidate buffer from its start: the first n records (default: all of it, with the guard's six)"""
        n = self.max_candidates + RAYS_GUARD_BYTES // RAY_CANDIDATE.itemsize if n is None else int(n)
        out = np.zeros(max(n, 1), RAY_CANDIDATE)
        self.ctx.check(self.lib.lmx_rays_read_candidates(self.ctx.h, _ptr(out), n))
        return out[:n]

    def deviceOutputs(self):
        """(d_hits, d_counts) device addresses"""
        h, c = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.lib.lmx_rays_device_outputs(self.ctx.h, C.byref(h), C.byref(c)))
        return h.value, c.value

    def setInstancedModels(self, im, ray_model=(), entity=()):
        """Attach an InstancedModels (None: detach): castRayInstancedModels runs ahead of every cast. ray_model[m] / entity[m]: the setModels
        model (-1: none) and the entity of the object's model m."""
        if im is None:
            self.ctx.check(self.lib.lmx_rays_set_instanced_models(self.ctx.h, None, 0, None, None))
            return
        rm = np.ascontiguousarray(ray_model, np.int32)
        en = np.ascontiguousarray(entity, np.int32)
        assert len(rm) == len(en)
        self.ctx.check(self.lib.lmx_rays_set_instanced_models(self.ctx.h, im.h, len(rm), _ptr(rm) if len(rm) else None, _ptr(en) if len(rm) else None))

    def imCounts(self) -> dict:
        c = np.zeros(1, RAYS_IM_COUNTS)
        self.ctx.check(self.lib.lmx_rays_im_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in RAYS_IM_COUNTS.names}

    def readImHits(self) -> np.ndarray:
        n = self.imCounts()["rays"]
        out = np.zeros(max(n, 1), RAY_IM_HIT)
        self.ctx.check(self.lib.lmx_rays_read_im_hits(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def deviceImOutputs(self):
        """(d_im_hits, d_im_counts) device addresses"""
        h, c = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.lib.lmx_rays_device_im_outputs(self.ctx.h, C.byref(h), C.byref(c)))
        return h.value, c.value

    def setProceduralGeometries(self, geometries):
        """castRayProceduralGeometry runs behind every cast ([] clears the table). geometries: dicts in m_procedural_geometries order with
        entity, aabb_min, aabb_max, vertex_data (any array: its bytes; empty: never cast), stride, indices (None, or a uint16 / uint32
        array), index_count (default: len(indices)) and triangles (default True: the primitive type is TRIANGLES)."""
        recs = np.zeros(len(geometries), RAY_PROC_GEOM)
        keep = []
        for r, g in zip(recs, geometries):
            v = np.frombuffer(np.ascontiguousarray(g["vertex_data"]).tobytes(), np.uint8)
            idx = g.get("indices")
            i = np.zeros(0, np.uint32) if idx is None else np.ascontiguousarray(idx).reshape(-1)
            keep += [v, i]
            r["entity"], r["triangles"] = g["entity"], 1 if g.get("triangles", True) else 0
            r["aabb_min"], r["aabb_max"] = g["aabb_min"], g["aabb_max"]
            r["vertex_data"], r["vertex_bytes"], r["stride"] = (v.ctypes.data if len(v) else 0), len(v), g["stride"]
            r["index_data"] = i.ctypes.data if len(i) else 0
            r["index_bytes"] = g.get("index_bytes", 0 if idx is None else i.dtype.itemsize)
            r["index_count"] = g.get("index_count", len(i))
        self.ctx.check(self.lib.lmx_rays_set_procedural_geometries(self.ctx.h, len(recs), _ptr(recs) if len(recs) else None))

    def setTerrains(self, terrains):
        """Terrain::castRay runs behind every cast for each terrain, in this (m_terrains) order ([] clears the table). terrains: dicts with
        entity, scale (x, y, z), heightmap ((height, width) uint16: R16, or uint32: RGBA8) and ready (default True)."""
        recs = np.zeros(len(terrains), RAY_TERRAIN)
        keep = []
        for r, t in zip(recs, terrains):
            h = np.ascontiguousarray(t["heightmap"])
            assert h.ndim == 2 and h.dtype in (np.uint16, np.uint32), (h.shape, h.dtype)
            keep.append(h)
            r["entity"], r["height"], r["width"] = t["entity"], h.shape[0], h.shape[1]
            r["format"] = t.get("format", RAY_TERRAIN_R16 if h.dtype == np.uint16 else RAY_TERRAIN_RGBA8)
            r["scale"], r["ready"], r["texels"] = t["scale"], 1 if t.get("ready", True) else 0, (h.ctypes.data if h.size else 0)
        self.ctx.check(self.lib.lmx_rays_set_terrains(self.ctx.h, len(recs), _ptr(recs) if len(recs) else None))
        self.n_terrains = len(recs)

    def sceneCounts(self) -> dict:
        c = np.zeros(1, RAYS_SCENE_COUNTS)
        self.ctx.check(self.lib.lmx_rays_scene_counts(self.ctx.h, _ptr(c)))
        return {k: int(c[k][0]) for k in RAYS_SCENE_COUNTS.names}

    def _read_scene(self, fn, dtype, per_ray=1):
        n = self.sceneCounts()["rays"] * per_ray
        out = np.zeros(max(n, 1), dtype)
        self.ctx.check(fn(self.ctx.h, _ptr(out), len(out)))
        return out[:n]

    def readPgHits(self) -> np.ndarray:
        return self._read_scene(self.lib.lmx_rays_read_pg_hits, RAY_PG_HIT)

    def readTerrainHits(self) -> np.ndarray:
        """(rays, terrains) records"""
        k = getattr(self, "n_terrains", 0)
        return self._read_scene(self.lib.lmx_rays_read_terrain_hits, RAY_TERRAIN_HIT, k).reshape(-1, k) if k else np.zeros((self.sceneCounts()["rays"], 0), RAY_TERRAIN_HIT)

    def readSceneHits(self) -> np.ndarray:
        """RenderModule::castRay's result per ray"""
        return self._read_scene(self.lib.lmx_rays_read_scene_hits, RAY_SCENE_HIT)

    def deviceSceneOutputs(self):
        """(d_scene_hits, d_scene_counts) device addresses"""
        h, c = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.lib.lmx_rays_device_scene_outputs(self.ctx.h, C.byref(h), C.byref(c)))
        return h.value, c.value


SKIN_FUSED, SKIN_EXACT, SKIN_DQS = 0, 1, 2


class Animators:
    """Animator controllers on the device (lmx_anim_controller_* / lmx_animators_*): one Animator per instance of `skinning`."""

    def __init__(self, skinning):
        self.ctx, self.lib, self.sk = skinning.ctx, skinning.lib, skinning
        self.n = 0

    @staticmethod
    def checkController(raw: bytes):
        """lmx_anim_controller_check (host only): (info record, enter image bytes). Raises LumixError(LMX_ERR_INVALID) with the parser's message."""
        lib = load_library()
        buf = np.frombuffer(bytes(raw), np.uint8)
        info = np.zeros(1, CONTROLLER_INFO)
        err = C.create_string_buffer(256)
        rc = lib.lmx_anim_controller_check(_ptr(buf) if len(buf) else None, len(buf), _ptr(info), None, 0, err, 256)
        if rc != 0:
            raise LumixError(rc, err.value.decode())
        image = np.zeros(max(int(info["enter_bytes"][0]), 1), np.uint8)
        rc = lib.lmx_anim_controller_check(_ptr(buf), len(buf), None, _ptr(image), len(image), err, 256)
        if rc != 0:
            raise LumixError(rc, err.value.decode())
        return info[0], image[: int(info["enter_bytes"][0])].tobytes()

    def addController(self, raw: bytes) -> int:
        buf = np.frombuffer(bytes(raw), np.uint8)
        out = _u32()
        self.ctx.check(self.lib.lmx_anim_controller_add(self.ctx.h, _ptr(buf) if len(buf) else None, len(buf), C.byref(out)))
        return int(out.value)

    def inputTypes(self, controller: int) -> np.ndarray:
        n = _u32()
        self.ctx.check(self.lib.lmx_anim_controller_input_types(self.ctx.h, controller, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.ctx.check(self.lib.lmx_anim_controller_input_types(self.ctx.h, controller, _ptr(out), len(out), C.byref(n)))
        return out[: n.value]

    def setSlots(self, controller: int, anim_set: int, slot_animation):
        a = np.ascontiguousarray(slot_animation, np.uint32)
        self.ctx.check(self.lib.lmx_anim_controller_set_slots(self.ctx.h, controller, anim_set, _ptr(a) if len(a) else None, len(a)))

    def setRootMotion(self, animation: int, translations=None, rotations=None):
        t = None if translations is None else np.ascontiguousarray(translations, np.float32)
        r = None if rotations is None else np.ascontiguousarray(rotations, np.float32)
        self.ctx.check(self.lib.lmx_anim_set_root_motion(self.ctx.h, animation, _ptr(t), _ptr(r)))

    def setAnimators(self, controller, anim_set, flags, entity, bone_hashes=None):
        c = np.ascontiguousarray(controller, np.uint32)
        s = np.ascontiguousarray(anim_set, np.uint32)
        f = np.ascontiguousarray(flags, np.uint32)
        e = np.ascontiguousarray(entity, np.int32)
        h = None if bone_hashes is None else np.ascontiguousarray(bone_hashes, np.uint64)
        self.ctx.check(self.lib.lmx_animators_set(self.ctx.h, len(c), _ptr(c), _ptr(s), _ptr(f), _ptr(e), _ptr(h), 0 if h is None else len(h)))
        self.n = len(c)

    def setInputs(self, first: int, n: int, values):
        v = np.ascontiguousarray(values, ANIMATOR_VALUE)
        self.ctx.check(self.lib.lmx_animators_set_inputs(self.ctx.h, first, n, _ptr(v) if len(v) else None))

    def setInputsDevice(self, first: int, n: int, device_ptr: int):
        self.ctx.check(self.lib.lmx_animators_set_inputs_device(self.ctx.h, first, n, C.c_void_p(device_ptr)))

    def update(self, time_delta: float):
        self.ctx.check(self.lib.lmx_animators_update(self.ctx.h, float(time_delta)))

    def readRootMotion(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), LOCAL_RIGID)
        self.ctx.check(self.lib.lmx_animators_read_root_motion(self.ctx.h, _ptr(out), self.n))
        return out[: self.n]

    def deviceOutputs(self):
        a, b, c = _vp(), _vp(), _vp()
        self.ctx.check(self.lib.lmx_animators_device_outputs(self.ctx.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def applyRootMotion(self):
        self.ctx.check(self.lib.lmx_animators_apply_root_motion(self.ctx.h))

    def readState(self, animator: int) -> bytes:
        n = _u32()
        self.ctx.check(self.lib.lmx_animators_read_state(self.ctx.h, animator, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 4), np.uint8)
        self.ctx.check(self.lib.lmx_animators_read_state(self.ctx.h, animator, _ptr(out), len(out), C.byref(n)))
        return out[: n.value].tobytes()

    def readInstrs(self):
        """(first_instr, BLEND_INSTR records) of the last update"""
        first = np.zeros(self.n + 1, np.uint32)
        n = _u32()
        self.ctx.check(self.lib.lmx_animators_read_instrs(self.ctx.h, _ptr(first), self.n, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), BLEND_INSTR)
        self.ctx.check(self.lib.lmx_animators_read_instrs(self.ctx.h, _ptr(first), self.n, _ptr(out), len(out), C.byref(n)))
        return first, out[: n.value]


class Skinning:
    """Pose -> palette -> skinned vertices for many model instances."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.lib = ctx.lib
        self._inst = []
        self._models = {}
        self._meshes = {}

    def addModel(self, parents, bind, first_nonroot: int) -> int:
        parents = np.ascontiguousarray(parents, np.int16)
        bind = np.ascontiguousarray(bind, LOCAL_RIGID)
        out = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_skin_add_model(self.ctx.h, len(parents), _ptr(parents), _ptr(bind), int(first_nonroot), C.byref(out)))
        self._models[out.value] = len(parents)
        return out.value

    def addMesh(self, positions, skin) -> int:
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        skin = np.ascontiguousarray(skin, SKIN)
        out = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_skin_add_mesh(self.ctx.h, len(positions), _ptr(positions), _ptr(skin), C.byref(out)))
        self._meshes[out.value] = len(positions)
        return out.value

    def setInstances(self, model, mesh):
        model = np.ascontiguousarray(model, np.uint32)
        mesh = np.ascontiguousarray(mesh, np.uint32)
        self._inst = [(int(a), int(b)) for a, b in zip(model, mesh)] if len(model) <= 4096 else None
        self._inst_model, self._inst_mesh = model, mesh
        self.ctx.check(self.lib.lmx_skin_set_instances(self.ctx.h, len(model), _ptr(model), _ptr(mesh)))

    def uploadPoses(self, positions, rotations):
        positions = np.ascontiguousarray(positions, np.float32)
        rotations = np.ascontiguousarray(rotations, np.float32)
        n_bones_total = positions.size // 3
        assert rotations.size == n_bones_total * 4
        self.ctx.check(self.lib.lmx_skin_upload_poses(self.ctx.h, _ptr(positions), _ptr(rotations), n_bones_total))

    def uploadPosesDevice(self, d_positions: int, d_rotations: int, n_bones_total: int):
        self.ctx.check(self.lib.lmx_skin_upload_poses_device(self.ctx.h, d_positions, d_rotations, n_bones_total))

    def setPoseSourceDevice(self, d_positions: Optional[int], d_rotations: Optional[int], n_bones_total: int):
        """run() reads the relative poses straight from this device memory (no copy) every time."""
        self.ctx.check(self.lib.lmx_skin_set_pose_source_device(self.ctx.h, d_positions, d_rotations, n_bones_total))

    def setMode(self, exact):
        """True / 1: FMA-free linear blend, bit-identical to the reference; False / 0 (default): fused multiply-adds, within 1e-5;
        2 (SKIN_DQS): the dual-quaternion blend of the reference's vertex shader."""
        self.ctx.check(self.lib.lmx_skin_set_mode(self.ctx.h, int(exact)))

    def setOption(self, option: int, value: int):
        """SKIN_OPT_INSTANCES_PER_BLOCK: 0 = k_skin_shared, 1 / 2 / 4 / 8 / 16 = k_skin_multi with that many instances per block."""
        self.ctx.check(self.lib.lmx_skin_set_option(self.ctx.h, int(option), int(value)))

    def run(self):
        self.ctx.check(self.lib.lmx_skin_run(self.ctx.h))

    def readVertices(self, instance: int) -> np.ndarray:
        n = self._meshes[int(self._inst_mesh[instance])]
        out = np.zeros((n, 3), np.float32)
        self.ctx.check(self.lib.lmx_skin_read_vertices(self.ctx.h, instance, _ptr(out), n))
        return out

    def readVerticesRange(self, first: int, count: int) -> np.ndarray:
        """Skinned positions of instances [first, first + count) in one copy: float32 [total vertices, 3], instances back to back."""
        n = int(sum(self._meshes[int(m)] for m in self._inst_mesh[first : first + count]))
        out = np.empty((n, 3), np.float32)
        self.ctx.check(self.lib.lmx_skin_read_vertices_range(self.ctx.h, first, count, _ptr(out), n))
        return out

    def deviceOutput(self):
        """(device pointer, total vertices) of the skinned positions in HBM (3 floats per vertex, instances back to back)."""
        p, n = C.c_void_p(), C.c_size_t()
        self.ctx.check(self.lib.lmx_skin_device_output(self.ctx.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def readPalette(self, instance: int) -> np.ndarray:
        n = self._models[int(self._inst_model[instance])]
        out = np.zeros(n, MATRIX)
        self.ctx.check(self.lib.lmx_skin_read_palette(self.ctx.h, instance, _ptr(out), n))
        return out

    # ---- animation sampling (AnimationModuleImpl::updateAnimable for every instance) ----
    def addAnimation(self, anim: dict) -> int:
        st, keep = animation_struct(anim)
        out = C.c_uint32(0)
        self.ctx.check(self.lib.lmx_anim_add(self.ctx.h, C.addressof(st), C.byref(out)))
        return out.value

    def setModelPose(self, model: int, relative):
        relative = np.ascontiguousarray(relative, LOCAL_RIGID)
        self.ctx.check(self.lib.lmx_anim_set_model_pose(self.ctx.h, model, _ptr(relative), len(relative)))

    def setAnimables(self, animation, time):
        animation, time = np.ascontiguousarray(animation, np.uint32), np.ascontiguousarray(time, np.uint32)
        self._n_animables = len(animation)
        self.ctx.check(self.lib.lmx_anim_set_animables(self.ctx.h, len(animation), _ptr(animation), _ptr(time)))

    def setAnimWeight(self, weight: float):
        self.ctx.check(self.lib.lmx_anim_set_weight(self.ctx.h, float(weight)))

    def updateAnimables(self, time_delta: float):
        self.ctx.check(self.lib.lmx_anim_update(self.ctx.h, float(time_delta)))

    def evalBlendStacks(self, stacks):
        """updateAnimator's pose work (animation_module.cpp:602-636): `stacks[i]` = instance i's SAMPLE instructions in order, each
        (animation id, weight, time, looped)."""
        first = np.zeros(len(stacks) + 1, np.uint32)
        first[1:] = np.cumsum([len(s) for s in stacks])
        samples = np.zeros(max(int(first[-1]), 1), BLEND_SAMPLE)
        k = 0
        for s in stacks:
            for (a, w, t, looped) in s:
                samples[k] = (a, w, t, 1 if looped else 0)
                k += 1
        self._n_animables = len(stacks)
        self.ctx.check(self.lib.lmx_anim_eval_blend_stacks(self.ctx.h, len(stacks), _ptr(first), _ptr(samples)))

    def evalBlendInstrs(self, programs):
        """evalBlendStack for every instance, IK included (lmx_anim_eval_blend_instrs): `programs[i]` = instance i's instructions in order,
        each ("sample", animation id, weight, time, looped) or ("ik", alpha, target xyz, leaf bone index or BONE_NONE, bones_count) - or a
        BLEND_INSTR array, as decodeBlendStack returns."""
        first = np.zeros(len(programs) + 1, np.uint32)
        first[1:] = np.cumsum([len(p) for p in programs])
        instrs = np.zeros(max(int(first[-1]), 1), BLEND_INSTR)
        k = 0
        for p in programs:
            if isinstance(p, np.ndarray):
                instrs[k : k + len(p)] = p
                k += len(p)
                continue
            for ins in p:
                if ins[0] == "sample":
                    instrs[k]["op"], instrs[k]["animation"], instrs[k]["weight"], instrs[k]["time"], instrs[k]["looped"] = BLEND_SAMPLE_OP, ins[1], ins[2], ins[3], 1 if ins[4] else 0
                elif ins[0] == "ik":
                    instrs[k]["op"], instrs[k]["alpha"], instrs[k]["target"], instrs[k]["leaf_bone"], instrs[k]["bones_count"] = BLEND_IK_OP, ins[1], ins[2], ins[3], ins[4]
                else:
                    instrs[k]["op"] = int(ins[0])  # (an unknown op, passed through for the library to refuse)
                k += 1
        self._n_animables = len(programs)
        self.ctx.check(self.lib.lmx_anim_eval_blend_instrs(self.ctx.h, len(programs), _ptr(first), _ptr(instrs)))

    @staticmethod
    def decodeBlendStack(blendstack: bytes, slot_animation, bone_hashes, weight: float = 1.0, capacity: int = 64) -> np.ndarray:
        """RuntimeContext::blendstack bytes -> BLEND_INSTR records (lmx_anim_decode_blend_stack; host only, no context). `slot_animation[slot]`
        = the library's animation id of RuntimeContext::animations[slot] (ANIM_NONE: empty), `bone_hashes` = the model's bone name hashes."""
        lib = load_library()
        raw = np.frombuffer(bytes(blendstack), np.uint8)
        slots = np.ascontiguousarray(slot_animation, np.uint32)
        hashes = np.ascontiguousarray(bone_hashes, np.uint64)
        out = np.zeros(max(capacity, 1), BLEND_INSTR)
        n = C.c_uint32(0)
        rc = lib.lmx_anim_decode_blend_stack(_ptr(raw) if len(raw) else None, len(raw), _ptr(slots) if len(slots) else None, len(slots),
                                             _ptr(hashes) if len(hashes) else None, len(hashes), float(weight), _ptr(out), int(capacity), C.byref(n))
        if rc != 0:
            raise LumixError(rc, "the blend stack could not be decoded")
        return out[: n.value].copy()

    def readTimes(self) -> np.ndarray:
        out = np.zeros(self._n_animables, np.uint32)
        self.ctx.check(self.lib.lmx_anim_read_times(self.ctx.h, _ptr(out), len(out)))
        return out

    def readRelativePose(self, instance: int):
        n = self._models[int(self._inst_model[instance])]
        pos, rot = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
        self.ctx.check(self.lib.lmx_anim_read_pose(self.ctx.h, instance, _ptr(pos), _ptr(rot), n))
        return pos, rot

    def blendPoses(self, positions, rotations, weight: float):
        """Pose::blend(rhs, weight) of the library's relative poses with `positions` / `rotations` (all instances back to back)."""
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        rotations = np.ascontiguousarray(rotations, np.float32).reshape(-1, 4)
        self.ctx.check(self.lib.lmx_skin_blend_poses(self.ctx.h, _ptr(positions), _ptr(rotations), len(positions), float(weight)))

    def setPoseWriteback(self, on: bool = True):
        """Store the absolute pose next to the palette (default) or not (readPose then fails)."""
        self.ctx.check(self.lib.lmx_skin_set_pose_writeback(self.ctx.h, int(on)))

    def enableDualQuats(self, on: bool = True):
        self.ctx.check(self.lib.lmx_skin_enable_dual_quats(self.ctx.h, int(on)))

    def readDualQuats(self, instance: int) -> np.ndarray:
        n = self._models[int(self._inst_model[instance])]
        out = np.zeros((n, 8), np.float32)
        self.ctx.check(self.lib.lmx_skin_read_dual_quats(self.ctx.h, instance, _ptr(out), n))
        return out

    def readPose(self, instance: int):
        n = self._models[int(self._inst_model[instance])]
        pos = np.zeros((n, 3), np.float32)
        rot = np.zeros((n, 4), np.float32)
        self.ctx.check(self.lib.lmx_skin_read_pose(self.ctx.h, instance, _ptr(pos), _ptr(rot), n))
        return pos, rot


PARTICLES_COUNTS = np.dtype([("particles", "<u4"), ("emit_index", "<u4"), ("overflow", "<u4"), ("killed", "<u4")])  # LmxParticlesCounts
PARTICLE_SLICE = np.dtype([("offset", "<u4"), ("bytes", "<u4"), ("particles", "<u4"), ("outputs_count", "<u4")])  # LmxParticleSlice
PARTICLE_RIBBON = np.dtype([("offset", "<u4"), ("length", "<u4"), ("emit_index", "<u4"), ("points_offset", "<u4")])  # LmxParticleRibbon
PARTICLES_GUARD_FLOATS = 64


class LmxParticleProgram(C.Structure):
    _fields_ = [("instructions", C.c_void_p), ("size", _u32), ("emit_offset", _u32), ("output_offset", _u32), ("channels_count", _u32), ("registers_count", _u32),
                ("outputs_count", _u32), ("emit_inputs_count", _u32), ("init_emit_count", _u32), ("emit_per_second", _f32)]


class LmxParticleEmitterOptions(C.Structure):
    _fields_ = [("max_ribbons", _u32), ("max_ribbon_length", _u32), ("init_ribbons_count", _u32), ("tube_segments", _u32), ("emit_move_distance", _f32)]


class LmxParticleMeshSource(C.Structure):
    _fields_ = [("mesh", _u32), ("skin_instance", _u32), ("flags", _u32)]


PARTICLE_MESH_HAS_BONES = 1


class LmxParticlesDevice(C.Structure):
    _fields_ = [("d_frame", C.c_void_p), ("d_slices", C.c_void_p), ("d_counts", C.c_void_p), ("n_emitters", _u32), ("frame_bytes", _u32)]


class ParticleSystems(_ContextObject):
    """ParticleSystem::update and Emitter::fillInstanceData of every registered system on the device (lmx_particles_*)."""

    UNIT = "particles"
    ALL = 0xFFFFFFFF

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.emitters = []  # (system, emitter) by global emitter index
        self.capacity = {}
        self.outputs = {}
        self._ribbon = {}

    def addSystem(self, n_emitters: int, n_globals: int = 0) -> int:
        s = _u32()
        self.ctx.check(self.lib.lmx_particles_add_system(self.h, n_emitters, n_globals, C.byref(s)))
        self.emitters += [(s.value, e) for e in range(n_emitters)]
        return s.value

    def setProgram(self, system: int, emitter: int, instructions: bytes, emit_offset: int, output_offset: int, channels_count: int, registers_count: int,
                   outputs_count: int, emit_inputs_count: int = 0, init_emit_count: int = 0, emit_per_second: float = 0.0):
        buf = np.frombuffer(bytes(instructions), np.uint8).copy() if len(instructions) else np.zeros(1, np.uint8)
        p = LmxParticleProgram(_ptr(buf), len(instructions), emit_offset, output_offset, channels_count, registers_count, outputs_count, emit_inputs_count,
                               init_emit_count, emit_per_second)
        self.ctx.check(self.lib.lmx_particles_set_program(self.h, system, emitter, C.byref(p)))
        self.outputs[(system, emitter)] = outputs_count

    def setGlobals(self, system: int, values):
        v = np.ascontiguousarray(values, np.float32)
        self.ctx.check(self.lib.lmx_particles_set_globals(self.h, system, _ptr(v) if len(v) else None, len(v)))

    def setEntityPositions(self, pos):
        p = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_particles_set_entity_positions(self.h, len(p), _ptr(p) if len(p) else None))

    def reserve(self, system: int, emitter: int, capacity: int):
        self.ctx.check(self.lib.lmx_particles_reserve(self.h, system, emitter, capacity))
        self.capacity[(system, emitter)] = (capacity + 3) & ~3

    def setEmitterOptions(self, system: int, emitter: int, max_ribbons: int = 0, max_ribbon_length: int = 0, init_ribbons_count: int = 0, tube_segments: int = 0,
                          emit_move_distance: float = 0.0):
        """What ParticleSystemResource::Emitter keeps next to its program; max_ribbons > 0 makes a ribbon emitter of fixed capacity."""
        o = LmxParticleEmitterOptions(max_ribbons, max_ribbon_length, init_ribbons_count, tube_segments, emit_move_distance)
        self.ctx.check(self.lib.lmx_particles_set_emitter_options(self.h, system, emitter, C.byref(o)))
        if max_ribbons:
            self.capacity[(system, emitter)] = max_ribbons * ((max_ribbon_length + 3) & ~3)
        elif self._ribbon.get((system, emitter)):
            self.capacity[(system, emitter)] = 0
        self._ribbon[(system, emitter)] = max_ribbons > 0

    def emitRibbons(self, system: int, emitter: int, n: int):
        self.ctx.check(self.lib.lmx_particles_emit_ribbons(self.h, system, emitter, n))

    def killRibbon(self, system: int, emitter: int, ribbon: int):
        self.ctx.check(self.lib.lmx_particles_kill_ribbon(self.h, system, emitter, ribbon))

    def applyTransforms(self, pos):
        """ParticleSystem::applyTransform of every system (positions only): emission on movement, and the entity positions."""
        p = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_particles_apply_transforms(self.h, len(p), _ptr(p) if len(p) else None))

    def ribbons(self, system: int, emitter: int) -> np.ndarray:
        """Emitter::ribbons with each ribbon's points_offset into the emitter's slice: host state, no wait."""
        n = _u32()
        self.lib.lmx_particles_ribbons(self.h, system, emitter, None, 0, C.byref(n))
        out = np.zeros(n.value, PARTICLE_RIBBON)
        self.ctx.check(self.lib.lmx_particles_ribbons(self.h, system, emitter, _ptr(out) if len(out) else None, len(out), C.byref(n)))
        return out

    # ---- what MESH and SPLINE read: declared per system before setProgram ----
    NONE = 0xFFFFFFFF

    def addMesh(self, positions, skin=None) -> int:
        """Mesh 0 of a model (positions [n, 3], optionally SKIN records); shared by every system whose source names it."""
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        sk = np.ascontiguousarray(skin, SKIN) if skin is not None else None
        assert sk is None or len(sk) == len(positions)
        out = _u32()
        self.ctx.check(self.lib.lmx_particles_add_mesh(self.h, len(positions), _ptr(positions) if len(positions) else None, _ptr(sk) if sk is not None else None,
                                                       C.byref(out)))
        return out.value

    def clearMeshes(self):
        self.ctx.check(self.lib.lmx_particles_clear_meshes(self.h))

    def setMeshSource(self, system: int, mesh: int = NONE, skin_instance: int = NONE, flags: int = 0):
        """The entity's model for MESH: a mesh of addMesh (NONE: no model), the skin instance whose palette Skinning.run left (NONE: no pose),
        PARTICLE_MESH_HAS_BONES."""
        src = LmxParticleMeshSource(mesh, skin_instance, flags)
        self.ctx.check(self.lib.lmx_particles_set_mesh_source(self.h, system, C.byref(src)))

    def setSpline(self, system: int, points=None):
        """The entity's spline for SPLINE ([n, 3], n >= 3); None or empty: no spline component."""
        p = np.ascontiguousarray(points if points is not None else [], np.float32).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_particles_set_spline(self.h, system, _ptr(p) if len(p) else None, len(p)))

    def reset(self, system: int = ALL):
        self.ctx.check(self.lib.lmx_particles_reset(self.h, system))

    def setSeed(self, seed: int):
        self.ctx.check(self.lib.lmx_particles_set_seed(self.h, seed))

    def update(self, dt: float):
        self.ctx.check(self.lib.lmx_particles_step(self.h, float(dt)))

    def fill(self):
        self.ctx.check(self.lib.lmx_particles_fill(self.h))

    def counts(self) -> np.ndarray:
        out = np.zeros(len(self.emitters), PARTICLES_COUNTS)
        self.ctx.check(self.lib.lmx_particles_counts(self.h, _ptr(out) if len(out) else None, len(out)))
        return out

    def readChannels(self, system: int, emitter: int, channels_count: int) -> np.ndarray:
        """[channels_count, capacity + guard] floats: the guard columns must still hold 0xA5 bytes."""
        stride = self.capacity.get((system, emitter), 0) + PARTICLES_GUARD_FLOATS
        out = np.zeros((channels_count, stride), np.float32)
        got = _u32()
        self.ctx.check(self.lib.lmx_particles_read_channels(self.h, system, emitter, _ptr(out) if out.size else None, out.size, C.byref(got)))
        assert got.value == stride
        return out

    def deviceOutputs(self) -> LmxParticlesDevice:
        d = LmxParticlesDevice()
        self.ctx.check(self.lib.lmx_particles_device_outputs(self.h, C.byref(d)))
        return d

    def readSlices(self):
        """(slice records by global emitter index, the frame buffer with its guard as float32)."""
        d = self.deviceOutputs()
        slices = np.zeros(len(self.emitters), PARTICLE_SLICE)
        data = np.zeros(d.frame_bytes // 4 + PARTICLES_GUARD_FLOATS, np.float32)
        self.ctx.check(self.lib.lmx_particles_read_slices(self.h, _ptr(slices) if len(slices) else None, len(slices), _ptr(data), data.nbytes))
        return slices, data


GRASS_TYPE = np.dtype([("spacing", "<f4"), ("distance", "<f4"), ("rotation_mode", "<u4"), ("usable", "<u4")])  # LmxGrassType
GRASS_TERRAIN = np.dtype([("heightmap", RAY_TERRAIN), ("splat_width", "<u4"), ("splat_height", "<u4"), ("splat_format", "<u4"), ("splat_ready", "<u4"),
                          ("splat_texels", "<u8"), ("types", "<u8"), ("n_types", "<u4"), ("_pad", "<u4")])  # LmxGrassTerrain
GRASS_INSTANCE = np.dtype([("position", "<f4", 3), ("scale", "<f4"), ("rotation", "<f4", 4)])  # LmxGrassInstance
GRASS_QUAD = np.dtype([("aabb_min", "<f4", 3), ("aabb_max", "<f4", 3), ("ij", "<i4", 2), ("type", "<u4"), ("instances_count", "<u4"), ("terrain", "<u4"), ("slot", "<u4")])  # LmxGrassQuad
GRASS_VIEW = np.dtype([("frustum", SHIFTED_FRUSTUM), ("viewport_pos", "<f8", 3), ("lod_multiplier", "<f4"), ("_pad", "<u4")])  # LmxGrassView
GRASS_DRAW = np.dtype([("quad", "<u4"), ("slot", "<u4"), ("terrain", "<u4"), ("type", "<u4"), ("instance_count", "<u4"), ("distance", "<f4")])  # LmxGrassDraw
GRASS_COUNTS = np.dtype([("draws", "<u4"), ("culled", "<u4"), ("instances", "<u4"), ("live", "<u4")])  # LmxGrassCounts
GRASS_ROTATION_Y_UP, GRASS_ROTATION_ALL_RANDOM = 0, 1  # LMX_GRASS_ROTATION_*
GRASS_MAX_TERRAINS, GRASS_MAX_TYPES, GRASS_SAMPLES, GRASS_SLOT_INSTANCES = 64, 16, 1024, 2048  # LMX_GRASS_*
GRASS_WINDOW = 64  # lmx_grass.h: texels per side of the splat window k_grass_quads stages in LDS
GRASS_CULL_BLOCK = 256
GRASS_ALL = 0xFFFFFFFF


class LmxGrassDevice(C.Structure):
    _fields_ = [("d_pool", C.c_void_p), ("d_quads", C.c_void_p), ("d_draws", C.c_void_p), ("d_counts", C.c_void_p), ("n_slots", _u32), ("draw_stride", _u32),
                ("n_views", _u32), ("n_live", _u32)]


class Grass(_ContextObject):
    """Terrain::createGrass of every terrain and renderGrass's quad loop of every view on the device (lmx_grass_*).

    A terrain is a dict: entity, heightmap (2-D uint16 = R16 or uint32 = RGBA8), scale (3), optional ready / format; splatmap (2-D uint32, or
    None), optional splat_format / splat_ready; types: a list of (spacing, distance, rotation_mode, usable)."""

    UNIT = "grass"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.n_terrains = 0
        self.n_views = 0

    def setTerrains(self, terrains):
        recs = np.zeros(len(terrains), GRASS_TERRAIN)
        keep = []
        for r, t in zip(recs, terrains):
            h = np.ascontiguousarray(t["heightmap"])
            keep.append(h)
            hm = r["heightmap"]
            hm["entity"] = t.get("entity", 0)
            hm["height"], hm["width"] = h.shape
            hm["format"] = t.get("format", RAY_TERRAIN_R16 if h.dtype == np.uint16 else RAY_TERRAIN_RGBA8)
            hm["scale"] = t["scale"]
            hm["ready"] = 1 if t.get("ready", True) else 0
            hm["texels"] = h.ctypes.data
            s = t.get("splatmap")
            if s is not None:
                s = np.ascontiguousarray(s, np.uint32)
                keep.append(s)
                r["splat_height"], r["splat_width"] = s.shape
                r["splat_texels"] = s.ctypes.data
            r["splat_format"] = t.get("splat_format", RAY_TERRAIN_RGBA8)
            r["splat_ready"] = 1 if t.get("splat_ready", True) else 0
            ty = np.zeros(len(t["types"]), GRASS_TYPE)
            for k, v in enumerate(t["types"]):
                ty[k] = tuple(v)
            keep.append(ty)
            r["types"] = ty.ctypes.data if len(ty) else 0
            r["n_types"] = len(ty)
        self.ctx.check(self.lib.lmx_grass_set_terrains(self.h, len(recs), _ptr(recs) if len(recs) else None))
        self.n_terrains = len(recs)

    def invalidate(self, terrain: int = GRASS_ALL):
        self.ctx.check(self.lib.lmx_grass_invalidate(self.h, terrain))

    def setPositions(self, pos):
        p = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        self.ctx.check(self.lib.lmx_grass_set_positions(self.h, len(p), _ptr(p) if len(p) else None))

    def reserve(self, slots: int):
        self.ctx.check(self.lib.lmx_grass_reserve(self.h, slots))
        self.n_slots = slots

    def update(self, frame: int, centers):
        c = np.ascontiguousarray(centers, np.float32).reshape(-1, 2)
        self.ctx.check(self.lib.lmx_grass_update(self.h, frame & 0xFFFFFFFF, len(c), _ptr(c) if len(c) else None))

    def cull(self, views):
        v = np.ascontiguousarray(views, GRASS_VIEW).reshape(-1)
        self.ctx.check(self.lib.lmx_grass_cull(self.h, len(v), _ptr(v) if len(v) else None))
        if len(v):
            self.n_views = len(v)

    def readQuads(self) -> np.ndarray:
        n = _u32()
        out = np.zeros(max(getattr(self, "n_slots", 0), 1), GRASS_QUAD)
        self.ctx.check(self.lib.lmx_grass_read_quads(self.h, _ptr(out), len(out), C.byref(n)))
        return out[: n.value]

    def readInstances(self, slot: int) -> np.ndarray:
        out = np.zeros(GRASS_SLOT_INSTANCES, GRASS_INSTANCE)
        self.ctx.check(self.lib.lmx_grass_read_instances(self.h, slot, _ptr(out), len(out)))
        return out

    def writeInstances(self, slot: int, records):
        r = np.ascontiguousarray(records, GRASS_INSTANCE).reshape(-1)
        self.ctx.check(self.lib.lmx_grass_write_instances(self.h, slot, _ptr(r) if len(r) else None, len(r)))

    def readDraws(self, view: int) -> np.ndarray:
        n = _u32()
        out = np.zeros(max(getattr(self, "n_slots", 0), 1), GRASS_DRAW)
        self.ctx.check(self.lib.lmx_grass_read_draws(self.h, view, _ptr(out), len(out), C.byref(n)))
        return out[: n.value]

    def counts(self) -> np.ndarray:
        out = np.zeros(max(self.n_views, 1), GRASS_COUNTS)
        self.ctx.check(self.lib.lmx_grass_counts(self.h, _ptr(out), len(out)))
        return out[: self.n_views]

    def deviceOutputs(self) -> LmxGrassDevice:
        d = LmxGrassDevice()
        self.ctx.check(self.lib.lmx_grass_device_outputs(self.h, C.byref(d)))
        return d


# ---- Voxels (renderer/voxels.cpp) ---------------------------------------------------------------------------------------
VOXELS_INFO = np.dtype([("aabb_min", "<f4", 3), ("aabb_max", "<f4", 3), ("voxel_size", "<f4"), ("resolution", "<i4", 3)])  # LmxVoxelsInfo
VOXEL_BLOCK, VOXEL_AO_LDS_WORDS = 256, 10240  # lmx_voxels.h (tests/test_isa_voxel_kernels.py holds them to the compiled kernels)
VOXEL_RNG_M_U, VOXEL_RNG_M_V = 36969 * 65536 - 1, 18000 * 65536 - 1
VOXELS_OPT_AO_LDS = 0  # LMX_VOXELS_OPT_AO_LDS


class LmxVoxelsMesh(C.Structure):
    _fields_ = [("positions", C.c_void_p), ("stride_bytes", _u32), ("n_vertices", _u32), ("indices", C.c_void_p), ("index_bytes", _u32), ("index_count", _u32)]


class LmxVoxelsDevice(C.Structure):
    _fields_ = [("d_voxels", C.c_void_p), ("d_ao", C.c_void_p), ("n_cells", _u32), ("pad", _u32)]


def voxels_grid(aabb_min, aabb_max, max_res: int) -> np.ndarray:
    """Voxels::beginRaster's arithmetic on the host (lmx_voxels_grid): one VOXELS_INFO record. Needs no device."""
    lib = load_library()
    out = np.zeros(1, VOXELS_INFO)
    rc = lib.lmx_voxels_grid(_ptr(_f32x3(aabb_min)), _ptr(_f32x3(aabb_max)), max_res, _ptr(out))
    if rc != 0:
        raise LumixError(rc, "lmx_voxels_grid refused the box")
    return out[0]


def voxels_rng_skip(u: int, v: int, n: int):
    """The generator's halves n draws behind (u, v) (lmx_voxels_rng_skip). Needs no device."""
    lib = load_library()
    uo, vo = _u32(), _u32()
    rc = lib.lmx_voxels_rng_skip(u, v, n, C.byref(uo), C.byref(vo))
    if rc != 0:
        raise LumixError(rc, "lmx_voxels_rng_skip")
    return uo.value, vo.value


def _voxel_mesh(positions, indices):
    """(positions: float32 (n, >= 3) rows - any row stride -, indices: uint16 or uint32) -> (LmxVoxelsMesh, the arrays it points into)"""
    p = np.asarray(positions)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] >= 3 and (len(p) == 0 or p.strides[1] == 4), "positions: float32 rows"
    i = np.ascontiguousarray(indices)
    assert i.dtype in (np.uint16, np.uint32), "indices: uint16 or uint32"
    i = i.reshape(-1)
    stride = p.strides[0] if len(p) else 12
    return LmxVoxelsMesh(p.ctypes.data if len(p) else None, stride, len(p), i.ctypes.data if len(i) else None, i.dtype.itemsize, len(i)), (p, i)


class Voxels(_ContextObject):
    """Voxels of renderer/voxels.cpp on the device (lmx_voxels_*): raster, computeAO, blurAO, the lookups and the importer's vertex bake."""

    UNIT = "voxels"

    def set(self, src: "Voxels"):
        self.ctx.check(self.lib.lmx_voxels_set(self.h, src.h))

    def beginRaster(self, aabb_min, aabb_max, max_res: int):
        self.ctx.check(self.lib.lmx_voxels_begin_raster(self.h, _ptr(_f32x3(aabb_min)), _ptr(_f32x3(aabb_max)), max_res))

    def raster(self, positions, indices):
        m, keep = _voxel_mesh(positions, indices)
        self.ctx.check(self.lib.lmx_voxels_raster(self.h, m.positions, m.stride_bytes, m.n_vertices, m.indices, m.index_bytes, m.index_count))

    def voxelize(self, meshes, max_res: int):
        """meshes: a list of (positions, indices)"""
        recs = (LmxVoxelsMesh * max(len(meshes), 1))()
        keep = []
        for k, (p, i) in enumerate(meshes):
            recs[k], arrays = _voxel_mesh(p, i)
            keep.append(arrays)
        self.ctx.check(self.lib.lmx_voxels_voxelize(self.h, C.cast(recs, C.c_void_p), len(meshes), max_res))

    def computeAO(self, ray_count: int, seed_u: int, seed_v: int):
        self.ctx.check(self.lib.lmx_voxels_compute_ao(self.h, ray_count, seed_u, seed_v))

    def rngState(self):
        u, v = _u32(), _u32()
        self.ctx.check(self.lib.lmx_voxels_rng_state(self.h, C.byref(u), C.byref(v)))
        return u.value, v.value

    def blurAO(self):
        self.ctx.check(self.lib.lmx_voxels_blur_ao(self.h))

    def setOption(self, option: int, value: int):
        self.ctx.check(self.lib.lmx_voxels_set_option(self.h, option, value))

    def sample(self, points, fill: int = 0xEE):
        """-> (voxel bytes, inside flags); a byte keeps `fill` where the point lies outside"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out, inside = np.full(len(p), fill, np.uint8), np.zeros(len(p), np.uint8)
        self.ctx.check(self.lib.lmx_voxels_sample(self.h, _ptr(p) if len(p) else None, len(p), _ptr(out), _ptr(inside)))
        return out, inside

    def sampleAO(self, points, fill: float = -7.0):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out, inside = np.full(len(p), fill, np.float32), np.zeros(len(p), np.uint8)
        self.ctx.check(self.lib.lmx_voxels_sample_ao(self.h, _ptr(p) if len(p) else None, len(p), _ptr(out), _ptr(inside)))
        return out, inside

    def bakeVertexAO(self, positions, min_ao: float, fill: int = 0xEE) -> np.ndarray:
        p = np.asarray(positions)
        assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] >= 3 and (len(p) == 0 or p.strides[1] == 4)
        out = np.full(len(p), fill, np.uint8)
        self.ctx.check(self.lib.lmx_voxels_bake_vertex_ao(self.h, p.ctypes.data if len(p) else None, p.strides[0] if len(p) else 12, len(p), min_ao, _ptr(out)))
        return out

    def info(self) -> np.ndarray:
        out = np.zeros(1, VOXELS_INFO)
        self.ctx.check(self.lib.lmx_voxels_info(self.h, _ptr(out)))
        return out[0]

    def _cells(self) -> int:
        r = self.info()["resolution"]
        return int(r[0]) * int(r[1]) * int(r[2])

    def read(self) -> np.ndarray:
        out = np.zeros(max(self._cells(), 1), np.uint8)
        self.ctx.check(self.lib.lmx_voxels_read(self.h, _ptr(out), len(out)))
        return out[: self._cells()]

    def readAO(self) -> np.ndarray:
        out = np.zeros(max(self._cells(), 1), np.float32)
        self.ctx.check(self.lib.lmx_voxels_read_ao(self.h, _ptr(out), len(out)))
        return out[: self._cells()]

    def deviceOutputs(self) -> LmxVoxelsDevice:
        d = LmxVoxelsDevice()
        self.ctx.check(self.lib.lmx_voxels_device_outputs(self.h, C.byref(d)))
        return d


# ---- Probe bake (EnvironmentProbePlugin, renderer/editor/render_plugins.cpp) -------------------------------------------
PROBES_MAX_BATCH_BYTES = 1 << 30  # LMX_PROBES_MAX_BATCH_BYTES
PROBE_BLOCK, SH_CHUNK, SH_STRIDE = 256, 256, 29  # lmx_probes.h (tests/test_isa_probe_kernels.py holds them to the compiled kernels)


class LmxProbesDevice(C.Structure):
    _fields_ = [("d_cubemaps", C.c_void_p), ("d_sh", C.c_void_p), ("d_mips", C.c_void_p), ("d_filtered", C.c_void_p), ("d_rgbm", C.c_void_p), ("n", _u32), ("size", _u32)]


def probes_batch_bytes(n: int, size: int) -> int:
    """The bytes of a batch of n cubemaps of one size, with lmx_probes_set_cubemaps' refusals (lmx_probes_batch_bytes). Needs no device."""
    lib = load_library()
    out = C.c_uint64()
    rc = lib.lmx_probes_batch_bytes(n, size, C.byref(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_probes_batch_bytes refused {n} cubemaps of size {size}")
    return out.value


def probe_mip_texels(size: int) -> int:
    """texels of mips 1 .. log2 size of one cubemap"""
    return sum(6 * (size >> m) ** 2 for m in range(1, size.bit_length()))


def probes_ggx_samples(level: int) -> np.ndarray:
    """ImportanceSampleGGX's tangent-space H of the 128 Hammersley points at roughness level / 4 (lmx_probes_ggx_samples). Needs no device."""
    lib = load_library()
    out = np.zeros((128, 3), np.float32)
    rc = lib.lmx_probes_ggx_samples(level, _ptr(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_probes_ggx_samples refused level {level}")
    return out


PROBE_LEVELS = 5  # roughness_levels


class ProbeBaker(_ContextObject):
    """The probe bake on the device (lmx_probes_*): SphericalHarmonics::compute, and the reflection probe's mip chain, radiance levels and
    RGBM bytes, for a batch of cubemaps."""

    UNIT = "probes"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.n = self.size = 0

    def setCubemaps(self, rgba):
        """rgba: float32 (n, 6, S, S, 4)"""
        a = np.ascontiguousarray(rgba, np.float32)
        assert a.ndim == 5 and a.shape[1] == 6 and a.shape[2] == a.shape[3] and a.shape[4] == 4, "cubemaps: (n, 6, S, S, 4)"
        self.ctx.check(self.lib.lmx_probes_set_cubemaps(self.h, a.shape[0], a.shape[2], _ptr(a) if a.size else None))
        self.n, self.size = a.shape[0], a.shape[2]

    def shRun(self):
        self.ctx.check(self.lib.lmx_probes_sh_run(self.h))

    def readSH(self) -> np.ndarray:
        """-> float32 (n, 9, 3): LmxEnvProbe::sh_coefs per probe"""
        out = np.zeros((max(self.n, 1), 9, 3), np.float32)
        self.ctx.check(self.lib.lmx_probes_read_sh(self.h, _ptr(out), len(out)))
        return out[: self.n]

    def mipsRun(self):
        self.ctx.check(self.lib.lmx_probes_mips_run(self.h))

    def readMips(self):
        """-> per probe a list of float32 (6, s, s, 4), mips 1 .. log2 S"""
        per = 4 * probe_mip_texels(self.size)
        out = np.zeros(max(self.n * per, 1), np.float32)
        self.ctx.check(self.lib.lmx_probes_read_mips(self.h, _ptr(out), out.size))
        res = []
        for p in range(self.n):
            at, mips = p * per, []
            for m in range(1, self.size.bit_length()):
                s = self.size >> m
                mips.append(out[at: at + 24 * s * s].reshape(6, s, s, 4))
                at += 24 * s * s
            res.append(mips)
        return res

    def filterRun(self):
        self.ctx.check(self.lib.lmx_probes_filter_run(self.h))

    def sample(self, probe: int, dirs, lods) -> np.ndarray:
        """the cube sampler alone: dirs (k, 3), lods (k,) -> float32 (k, 3)"""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        l = np.ascontiguousarray(lods, np.float32).reshape(-1)
        assert len(d) == len(l)
        out = np.zeros((max(len(d), 1), 3), np.float32)
        self.ctx.check(self.lib.lmx_probes_sample(self.h, probe, len(d), _ptr(d) if len(d) else None, _ptr(l) if len(l) else None, _ptr(out)))
        return out[: len(d)]

    def _level_texels(self) -> int:
        return sum(6 * (self.size >> k) ** 2 for k in range(PROBE_LEVELS))

    def readFiltered(self):
        """-> per probe a list of float32 (6, s, s, 4), levels 0 .. 4"""
        per = 4 * self._level_texels()
        out = np.zeros(max(self.n * per, 1), np.float32)
        self.ctx.check(self.lib.lmx_probes_read_filtered(self.h, _ptr(out), out.size))
        res = []
        for p in range(self.n):
            at, levels = p * per, []
            for k in range(PROBE_LEVELS):
                s = self.size >> k
                levels.append(out[at: at + 24 * s * s].reshape(6, s, s, 4))
                at += 24 * s * s
            res.append(levels)
        return res

    def readRGBM(self):
        """-> per probe, per face a list of uint8 (s, s, 4), levels 0 .. 4: the images of TextureCompressor::Input::add(face, 0, level)"""
        per = 4 * self._level_texels()
        out = np.zeros(max(self.n * per, 1), np.uint8)
        self.ctx.check(self.lib.lmx_probes_read_rgbm(self.h, _ptr(out), out.size))
        res = []
        for p in range(self.n):
            at, faces = p * per, []
            for f in range(6):
                levels = []
                for k in range(PROBE_LEVELS):
                    s = self.size >> k
                    levels.append(out[at: at + 4 * s * s].reshape(s, s, 4))
                    at += 4 * s * s
                faces.append(levels)
            res.append(faces)
        return res

    def deviceOutputs(self) -> LmxProbesDevice:
        d = LmxProbesDevice()
        self.ctx.check(self.lib.lmx_probes_device_outputs(self.h, C.byref(d)))
        return d


# ---- texture compressor (lmx_texcomp_*) ---------------------------------------------------------------------------------------------------
TEX_BC1, TEX_BC3, TEX_BC4, TEX_BC5 = 0, 1, 2, 3
TEX_BLOCK_BYTES = {TEX_BC1: 8, TEX_BC3: 16, TEX_BC4: 8, TEX_BC5: 16}
TEXCOMP_GUARD_BYTES = 256  # behind the blocks of a run (a larger read returns them: 0xA5 each)


class LmxTexCompDevice(C.Structure):
    _fields_ = [("d_rgba", C.c_void_p), ("d_blocks", C.c_void_p), ("bytes", C.c_uint64), ("n_images", _u32), ("n_blocks", _u32), ("format", C.c_int32)]


# lmx_texcomp_tables' bytes: TcTables of csrc/lmx_texcomp.h
_TEX_HIST = np.dtype([("f", "<u4"), ("iz00", "<f4"), ("iz10", "<f4"), ("iz11", "<f4")])
TEX_TABLES = np.dtype([("hist4", _TEX_HIST, (969,)), ("hist3", _TEX_HIST, (153,)), ("mid5", "<f4", (32,)), ("mid6", "<f4", (64,)), ("match", "<u4", (4, 256))])


def _tex_descs(sizes) -> np.ndarray:
    d = np.ascontiguousarray(np.asarray(sizes, dtype=np.uint32).reshape(-1, 2))  # rows of (w, h)
    return d


def texcomp_output_bytes(sizes, fmt: int) -> int:
    """The bytes a run of `fmt` leaves for images of these (w, h), with the sets' refusals (lmx_texcomp_output_bytes). Needs no device."""
    lib = load_library()
    d = _tex_descs(sizes)
    out = C.c_uint64()
    rc = lib.lmx_texcomp_output_bytes(len(d), _ptr(d) if len(d) else None, fmt, C.byref(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_texcomp_output_bytes refused {len(d)} images, format {fmt}")
    return out.value


def texcomp_blocks_per_round() -> int:
    """The blocks the search kernel's largest grid takes in one round; more are walked with that stride (lmx_texcomp_blocks_per_round). Needs no device."""
    return int(load_library().lmx_texcomp_blocks_per_round())


def texcomp_tables() -> np.ndarray:
    """The generated tables (lmx_texcomp_tables) as one record of TEX_TABLES. Needs no device."""
    lib = load_library()
    out = np.zeros(1, TEX_TABLES)
    rc = lib.lmx_texcomp_tables(_ptr(out), out.nbytes)
    if rc != 0:
        raise LumixError(rc, "lmx_texcomp_tables failed")
    return out[0]


def texcomp_hist_index(hist) -> int:
    """The place of a histogram of 4 or 3 counts in the order the search tries them in (lmx_texcomp_hist_index). Needs no device."""
    lib = load_library()
    h = np.ascontiguousarray(hist, np.uint8)
    out = _u32()
    rc = lib.lmx_texcomp_hist_index(len(h), _ptr(h), C.byref(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_texcomp_hist_index refused {h.tolist()}")
    return out.value


def texcomp_encode_host(fmt: int, blocks):
    """The kernels' arithmetic on the host (lmx_texcomp_encode_host): blocks uint8 (n, 16, 4) -> (uint8 (n, bytes per block), uint32 (n,) errors)."""
    lib = load_library()
    px = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16, 4)
    out = np.zeros((len(px), TEX_BLOCK_BYTES.get(fmt, 16)), np.uint8)
    err = np.zeros(max(len(px), 1), np.uint32)
    rc = lib.lmx_texcomp_encode_host(fmt, len(px), _ptr(px) if len(px) else _ptr(err), _ptr(out) if len(px) else _ptr(err), _ptr(err))
    if rc != 0:
        raise LumixError(rc, f"lmx_texcomp_encode_host refused format {fmt}")
    return out, err[: len(px)]


# mip chains (csrc/lmx_texmips.h)
TEXMIP_LINEAR, TEXMIP_SRGB, TEXMIP_STOCHASTIC = 0, 1, 2
TEXMIP_MAX_TAPS = 14
TEXMIP_ROW = np.dtype([("n0", "<u4"), ("n", "<u4"), ("c", "<f4", (TEXMIP_MAX_TAPS,))])  # lmx_texmips_coeffs' records


class LmxTexMipOptions(C.Structure):
    _fields_ = [("mode", C.c_int32), ("scale_coverage_ref", C.c_float)]


def texcomp_chain_levels(w: int, h: int) -> int:
    """1 + log2(max(w, h)), the levels of a w x h chain (lmx_texcomp_chain_levels). Needs no device."""
    return int(load_library().lmx_texcomp_chain_levels(w, h))


def texcomp_chain_sizes(w: int, h: int):
    """the (w, h) of every level of a chain"""
    return [(max(w >> m, 1), max(h >> m, 1)) for m in range(texcomp_chain_levels(w, h))]


def texcomp_chain_bytes(n: int, w: int, h: int) -> int:
    """The bytes of n chains of w x h RGBA8, with set_chains' refusals (lmx_texcomp_chain_bytes). Needs no device."""
    out = C.c_uint64()
    rc = load_library().lmx_texcomp_chain_bytes(n, w, h, C.byref(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_texcomp_chain_bytes refused {n} chains of {w} x {h}")
    return out.value


def texmips_coeffs(n_in: int, n_out: int) -> np.ndarray:
    """The taps of one axis of a filtered level (lmx_texmips_coeffs): n_out records of TEXMIP_ROW. Needs no device."""
    rows = np.zeros(max(n_out, 1), TEXMIP_ROW)
    rc = load_library().lmx_texmips_coeffs(n_in, n_out, _ptr(rows), len(rows))
    if rc != 0:
        raise LumixError(rc, f"lmx_texmips_coeffs refused {n_in} -> {n_out}")
    return rows[:n_out]


def texmips_host(images, mode: int, scale_coverage_ref: float = -1.0) -> np.ndarray:
    """The chains' arithmetic on the host (lmx_texmips_host): images uint8 (n, h, w, 4) -> uint8 (n, chain bytes)."""
    px = np.ascontiguousarray(images, np.uint8)
    assert px.ndim == 4 and px.shape[3] == 4, "images: (n, h, w, 4)"
    n, h, w = px.shape[:3]
    out = np.zeros((n, texcomp_chain_bytes(n, w, h) // n), np.uint8)
    opt = LmxTexMipOptions(mode, scale_coverage_ref)
    rc = load_library().lmx_texmips_host(C.byref(opt), n, w, h, _ptr(px), _ptr(out))
    if rc != 0:
        raise LumixError(rc, f"lmx_texmips_host refused mode {mode}, {n} x {w} x {h}")
    return out


def texcomp_split_chain(chain, w: int, h: int):
    """one chain's bytes -> its levels, uint8 (h_m, w_m, 4) each"""
    flat, at, out = np.asarray(chain, np.uint8).reshape(-1), 0, []
    for lw, lh in texcomp_chain_sizes(w, h):
        out.append(flat[at: at + 4 * lw * lh].reshape(lh, lw, 4))
        at += 4 * lw * lh
    return out


class TexCompressor(_ContextObject):
    """TextureCompressor::compress's block loops on the device (lmx_texcomp_*): BC1, BC3, BC4 and BC5 blocks of a batch of RGBA8 images,
    and the mip chains of compress() with generate_mipmaps (setChains, generateMips)."""

    UNIT = "texcomp"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.sizes = np.zeros((0, 2), np.uint32)
        self.format = -1

    def setImages(self, images):
        """images: a list of uint8 (h, w, 4)"""
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        assert all(im.ndim == 3 and im.shape[2] == 4 for im in imgs), "images: (h, w, 4)"
        d = _tex_descs([(im.shape[1], im.shape[0]) for im in imgs])
        flat = np.concatenate([im.reshape(-1) for im in imgs]) if imgs else np.zeros(0, np.uint8)
        self.ctx.check(self.lib.lmx_texcomp_set_images(self.h, len(d), _ptr(d) if len(d) else None, _ptr(flat) if flat.size else None))
        self.sizes, self.format = d, -1

    def setImagesDevice(self, sizes, d_rgba: int):
        """sizes: rows of (w, h); d_rgba: a device address of the tightly packed pixels (not copied)"""
        d = _tex_descs(sizes)
        self.ctx.check(self.lib.lmx_texcomp_set_images_device(self.h, len(d), _ptr(d) if len(d) else None, C.c_void_p(d_rgba)))
        self.sizes, self.format = d, -1

    def setFromProbes(self, baker: "ProbeBaker"):
        self.ctx.check(self.lib.lmx_texcomp_set_from_probes(self.h, baker.h))
        self.sizes = _tex_descs([(baker.size >> k, baker.size >> k) for _ in range(baker.n) for _ in range(6) for k in range(PROBE_LEVELS)])
        self.format = -1

    def setChains(self, images):
        """images: uint8 (n, h, w, 4), the level-0 images in slice, face order; the batch becomes n x levels images in (image, mip) order"""
        px = np.ascontiguousarray(images, np.uint8)
        assert px.ndim == 4 and px.shape[3] == 4, "images: (n, h, w, 4)"
        n, h, w = px.shape[:3]
        self.ctx.check(self.lib.lmx_texcomp_set_chains(self.h, n, w, h, _ptr(px) if px.size else None))
        self._chains_set(n, w, h)

    def setChainsDevice(self, n: int, w: int, h: int, d_rgba: int):
        """d_rgba: a device address of the n tightly packed level-0 images (copied on the stream)"""
        self.ctx.check(self.lib.lmx_texcomp_set_chains_device(self.h, n, w, h, C.c_void_p(d_rgba)))
        self._chains_set(n, w, h)

    def _chains_set(self, n, w, h):
        self.chain = (n, w, h)
        self.sizes, self.format = _tex_descs(texcomp_chain_sizes(w, h) * n), -1

    def generateMips(self, mode: int, scale_coverage_ref: float = -1.0):
        opt = LmxTexMipOptions(mode, scale_coverage_ref)
        self.ctx.check(self.lib.lmx_texcomp_generate_mips(self.h, C.byref(opt)))
        self.format = -1

    def readPixels(self, guard: bool = False) -> np.ndarray:
        """-> uint8 (n, chain bytes): every chain's levels one behind the other; guard: (bytes + TEXCOMP_GUARD_BYTES,) with what lies behind"""
        n, w, h = getattr(self, "chain", (0, 0, 0))
        total = texcomp_chain_bytes(n, w, h) if n else 0
        out = np.zeros(max(total, 1) + (TEXCOMP_GUARD_BYTES if guard else 0), np.uint8)
        self.ctx.check(self.lib.lmx_texcomp_read_pixels(self.h, _ptr(out), out.size))
        return out if guard else out[:total].reshape(n, total // n)

    def run(self, fmt: int):
        self.ctx.check(self.lib.lmx_texcomp_run(self.h, fmt))
        self.format = fmt

    def blockCounts(self) -> np.ndarray:
        return ((self.sizes[:, 0] + 3) >> 2) * ((self.sizes[:, 1] + 3) >> 2)

    def read(self, guard: bool = False) -> np.ndarray:
        """-> uint8 (blocks, bytes per block) of the last run, images one behind the other; guard: (bytes + TEXCOMP_GUARD_BYTES,) with what lies behind"""
        per = TEX_BLOCK_BYTES.get(self.format, 16)
        n = int(self.blockCounts().sum()) if self.format >= 0 else 0
        out = np.zeros(max(n * per, 1) + (TEXCOMP_GUARD_BYTES if guard else 0), np.uint8)
        self.ctx.check(self.lib.lmx_texcomp_read(self.h, _ptr(out), out.size))
        return out if guard else out[: n * per].reshape(n, per)

    def deviceOutputs(self) -> LmxTexCompDevice:
        d = LmxTexCompDevice()
        self.ctx.check(self.lib.lmx_texcomp_device_outputs(self.h, C.byref(d)))
        return d


# ---- animation compressor (lmx_animcomp_*) --------------------------------------------------------------------------------------------------
ANIM_KEY = np.dtype([("pos", "<f4", 3), ("rot", "<f4", 4)])  # LmxAnimKey
ANIMCOMP_STATUS = {0: "OK", 1: "NO_SAMPLES", 2: "BAD_ERROR", 3: "NONFINITE_BIND", 4: "NONFINITE_KEY", 5: "QUOTIENT_RANGE", 6: "CHANNEL_BITS", 7: "ENTRY_BITS", 8: "FRAME_BITS"}  # LMX_ANIMCOMP_*
ANIMCOMP_GUARD_BYTES = 256  # behind the streams of a run


class LmxAnimCompClip(C.Structure):
    _fields_ = [("n_bones", C.c_uint32), ("n_samples", C.c_uint32), ("fps", C.c_float), ("translation_error", C.c_float), ("rotation_error", C.c_float),
                ("_pad", C.c_uint32), ("has_keys", C.c_void_p), ("bind_positions", C.c_void_p), ("key_offset", C.c_uint64)]


class LmxAnimCompInfo(C.Structure):
    _fields_ = [("n_const_translations", C.c_uint32), ("n_translations", C.c_uint32), ("n_const_rotations", C.c_uint32), ("n_rotations", C.c_uint32),
                ("translations_frame_size_bits", C.c_uint32), ("rotations_frame_size_bits", C.c_uint32), ("translation_stream_size", C.c_uint64),
                ("rotation_stream_size", C.c_uint64), ("frame_count", C.c_uint32), ("status", C.c_uint32)]


class LmxAnimCompOutput(C.Structure):
    _fields_ = [("const_translations", C.c_void_p), ("translations", C.c_void_p), ("const_rotations", C.c_void_p), ("rotations", C.c_void_p),
                ("translation_stream", C.c_void_p), ("rotation_stream", C.c_void_p), ("cap_tracks", C.c_uint32), ("_pad", C.c_uint32),
                ("cap_translation_stream", C.c_uint64), ("cap_rotation_stream", C.c_uint64)]


class LmxAnimCompDevice(C.Structure):
    _fields_ = [("d_keys", C.c_void_p), ("d_infos", C.c_void_p), ("d_const_translations", C.c_void_p), ("d_translations", C.c_void_p), ("d_const_rotations", C.c_void_p),
                ("d_rotations", C.c_void_p), ("d_translation_streams", C.c_void_p), ("d_rotation_streams", C.c_void_p), ("n_clips", C.c_uint32), ("n_bones", C.c_uint32)]


def _animcomp_descs(clips):
    """clips: dicts of keys (n_samples, n_bones) ANIM_KEY, bind (n_bones, 3), optional has_keys (n_bones,), fps, translation_error, rotation_error
    -> (the descriptor array, all records one clip behind the other, keep-alive list)"""
    descs = (LmxAnimCompClip * max(len(clips), 1))()
    keep, flat, at = [], [], 0
    for i, c in enumerate(clips):
        keys = np.ascontiguousarray(c["keys"], ANIM_KEY)
        assert keys.ndim == 2, "keys: (n_samples, n_bones)"
        bind = np.ascontiguousarray(c["bind"], np.float32).reshape(keys.shape[1], 3)
        has = None if c.get("has_keys") is None else np.ascontiguousarray(c["has_keys"], np.uint8).reshape(keys.shape[1])
        keep += [bind, has]
        descs[i] = LmxAnimCompClip(keys.shape[1], keys.shape[0], float(c.get("fps", 30.0)), float(c.get("translation_error", 1.0)), float(c.get("rotation_error", 1.0)), 0,
                                   _ptr(has), _ptr(bind), at)
        flat.append(keys.reshape(-1))
        at += keys.size
    records = np.concatenate(flat) if flat else np.zeros(0, ANIM_KEY)
    if records.size == 0:
        records = np.zeros(1, ANIM_KEY)  # (a non-null pointer for a batch of clips without samples)
    return descs, records, keep


def _animcomp_result(info: LmxAnimCompInfo):
    """the info as a dict, and arrays with room for the clip's tables and streams"""
    d = {name: int(getattr(info, name)) for name, _ in LmxAnimCompInfo._fields_}
    arrays = [np.zeros(d["n_const_translations"], ANIM_CONST_TRANSLATION), np.zeros(d["n_translations"], ANIM_TRANSLATION_TRACK),
              np.zeros(d["n_const_rotations"], ANIM_CONST_ROTATION), np.zeros(d["n_rotations"], ANIM_ROTATION_TRACK),
              np.zeros(d["translation_stream_size"], np.uint8), np.zeros(d["rotation_stream_size"], np.uint8)]
    out = LmxAnimCompOutput(*[_ptr(a) if a.size else None for a in arrays], max(len(a) for a in arrays[:4]), 0, arrays[4].size, arrays[5].size)
    d.update(zip(("const_translations", "translations", "const_rotations", "rotations", "translation_stream", "rotation_stream"), arrays))
    return d, out


def animcomp_compress_host(clip: dict) -> dict:
    """One clip with the kernels' arithmetic on the host (lmx_animcomp_compress_host): the info's fields, and for a clip that was not refused
    its four tables and two streams. Needs no device."""
    lib = load_library()
    descs, records, keep = _animcomp_descs([clip])
    info = LmxAnimCompInfo()
    rc = lib.lmx_animcomp_compress_host(C.byref(descs[0]), _ptr(records), C.byref(info), None)
    if rc != 0:
        raise LumixError(rc, "lmx_animcomp_compress_host refused the clip's descriptor")
    d, out = _animcomp_result(info)
    if d["status"] == 0:
        rc = lib.lmx_animcomp_compress_host(C.byref(descs[0]), _ptr(records), C.byref(info), C.byref(out))
        if rc != 0:
            raise LumixError(rc, "lmx_animcomp_compress_host: the arrays sized from its own info are too small")
    return d


def animcomp_animation(result: dict, fps: float, length: int) -> dict:
    """a compressed clip as the dict animation_struct takes, without root motion"""
    a = {k: result[k] for k in ("const_translations", "translations", "const_rotations", "rotations", "translation_stream", "rotation_stream",
                                "frame_count", "translations_frame_size_bits", "rotations_frame_size_bits")}
    a.update(fps=fps, length=length, root_translation_track=-1, root_rotation_track=-1, root_pose_translations=np.zeros(0, np.float32), root_pose_rotations=np.zeros(0, np.float32))
    return a


class AnimCompressor(_ContextObject):
    """ModelImporter::writeAnimations' loops on the device (lmx_animcomp_*): a batch of clips of sampled keys -> each clip's track tables and
    its two bit streams."""

    UNIT = "animcomp"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self.n = 0

    def setClips(self, clips):
        """clips: see _animcomp_descs"""
        descs, records, keep = _animcomp_descs(clips)
        self.ctx.check(self.lib.lmx_animcomp_set_clips(self.h, len(clips), C.byref(descs) if len(clips) else None, _ptr(records)))
        self.n = len(clips)

    def setClipsDevice(self, clips, d_keys: int):
        """the same with the records of all clips, one clip behind the other, at the device address d_keys (not copied); the dicts' keys
        give the shapes"""
        descs, records, keep = _animcomp_descs(clips)
        self.ctx.check(self.lib.lmx_animcomp_set_clips_device(self.h, len(clips), C.byref(descs) if len(clips) else None, C.c_void_p(d_keys)))
        self.n = len(clips)

    def run(self):
        self.ctx.check(self.lib.lmx_animcomp_run(self.h))

    def clipInfo(self, clip: int) -> dict:
        info = LmxAnimCompInfo()
        self.ctx.check(self.lib.lmx_animcomp_clip_info(self.h, clip, C.byref(info)))
        return _animcomp_result(info)[0]

    def readClip(self, clip: int) -> dict:
        """the info's fields, and for a clip that was not refused its four tables and two streams"""
        info = LmxAnimCompInfo()
        self.ctx.check(self.lib.lmx_animcomp_clip_info(self.h, clip, C.byref(info)))
        d, out = _animcomp_result(info)
        if d["status"] == 0:
            self.ctx.check(self.lib.lmx_animcomp_read_clip(self.h, clip, C.byref(out)))
        return d

    def addTo(self, clip: int, length: int) -> int:
        """lmx_anim_add_compressed: the clip into the context's animation tables, its streams copied device to device -> the animation's id"""
        out = C.c_uint32()
        self.ctx.check(self.lib.lmx_anim_add_compressed(self.ctx.h, self.h, clip, length, C.byref(out)))
        return int(out.value)

    def deviceOutputs(self):
        """-> (LmxAnimCompDevice, bone_offset (n,), translation_offset (n,), rotation_offset (n,))"""
        d = LmxAnimCompDevice()
        bone, t_at, r_at = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint64), np.zeros(max(self.n, 1), np.uint64)
        self.ctx.check(self.lib.lmx_animcomp_device_outputs(self.h, C.byref(d), _ptr(bone), _ptr(t_at), _ptr(r_at)))
        return d, bone[: self.n], t_at[: self.n], r_at[: self.n]
