"""numpy restatement of the model-instance loop of RenderModuleImpl::castRay (renderer/render_module.cpp:2715-2759) with Model::castRay
(renderer/model.cpp:139-223), evaluateSkin (model.cpp:103-109), getRaySphereIntersection / getRayAABBIntersection (core/geometry.cpp:844-889)
and the Transform members they call (core/math.cpp:765-797).

Written from the description of the algorithm, line by line cited, with none of the reference's text. Every product, sum, quotient and
root is one np.float32 or np.float64 step (numpy never fuses), in the reference's operation order. Two forms:

  cast_sequential  the reference's walk: entities in index order, the distance gate against the nearest hit so far (`cur_dist`), a later
                   entity replaces the hit when its new_t is strictly smaller;
  cast             the order-free form the device computes: the distance gate against the ray's t_max only, per ray the entity of smallest
                   new_t (ties: the smallest index), a NaN model-space t is no hit.

agrees(scene, rays) says whether the two give the same hits; a scene for the device tests must make it true.

A scene is a dict:
  meshes      list of {"positions": (n, 3) f32, "indices": uint16 / uint32 (3 k,), "skin": api.SKIN array or None}
  models      api.RAY_MODEL array (first_mesh / mesh_count index `meshes`)
  inst_model  int32 per entity (-1: none), inst_flags uint8 per entity
  transforms  api.TRANSFORM array by entity (an entity past it reads as zero)
  palettes    {entity: (n_bones, 4, 4) f32, columns[c][r]} - the skin matrices of the entity's pose; absent: no pose
"""
import numpy as np

f32, f64 = np.float32, np.float64
ENABLED, VALID = 1 << 1, 1 << 2  # ModelInstance::Flags, render_module.h:209-212
HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("mesh", "<u4"), ("triangle", "<u4"), ("t", "<f4"), ("t_model", "<f4")])


def _cross(a, b):  # core/math.cpp:1274-1280, columns of (..., 3) arrays
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):  # core/math.cpp:1266-1268
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _rotate(q, v, ty):  # Quat::rotate, core/math.cpp:164-188; q (..., 4) f32, v (..., 3) of type ty
    qv = q[..., :3].astype(ty)
    uv = _cross(qv, v)
    uuv = _cross(qv, uv)
    uv = uv * (ty(2) * q[..., 3:4].astype(ty))
    uuv = uuv * ty(2)
    return (v + uv) + uuv


def _conj(q):  # core/math.cpp:664-667
    return np.concatenate([q[..., :3], -q[..., 3:4]], -1)


def _safe_inv(s):  # core/math.cpp:9-12
    with np.errstate(all="ignore"):
        return np.where(s == 0, f32(0), f32(1) / s).astype(f32)


def _minimum(a, b):  # core/math.h:420-422
    return np.where(a < b, a, b)


def _maximum(a, b):  # core/math.h:472-475
    return np.where(a > b, a, b)


def _transforms(scene, n):
    tr = scene["transforms"]
    pos, rot, scale = np.zeros((n, 3), f64), np.zeros((n, 4), f32), np.zeros((n, 3), f32)
    k = min(n, len(tr))
    pos[:k], rot[:k], scale[:k] = tr["pos"][:k], tr["rot"][:k], tr["scale"][:k]
    return pos, rot, scale


def _broad(scene, ray, tr):
    """Steps 1, 2, 4, 5, 6 for every entity at once -> (passes, dist - reach, o, d); the distance gate is left to the caller."""
    pos, rot, scale = tr
    n = len(scene["inst_model"])
    models = scene["models"]
    model = np.asarray(scene["inst_model"], np.int64)
    has = (np.asarray(scene["inst_flags"], np.uint8) & (ENABLED | VALID)) != 0
    has &= (model >= 0) & (model < len(models))
    m = np.where(has, model, 0)
    if len(models) == 0:
        return np.zeros(n, bool), np.zeros(n, f64), np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    has &= models["ready"][m] != 0
    if ray["ignore"] >= 0:
        has &= np.arange(n) != ray["ignore"]
    radius = models["origin_radius"][m].astype(f32)
    origin = ray["origin"].astype(f64)
    with np.errstate(all="ignore"):
        dp = pos - origin
        dist = np.sqrt(dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2])  # :2730, core/math.cpp:393
        reach = radius * _maximum(scale[:, 0], _maximum(scale[:, 1], scale[:, 2]))  # f32; core/math.h:472-475: a > max(b, c) ? a : max(b, c)
        gate = dist - reach.astype(f64)
        inv = _safe_inv(scale)
        rotated = _rotate(_conj(rot), origin - pos, f64)  # Transform::invTransform(DVec3), core/math.cpp:767-774
        o = (rotated * inv.astype(f64)).astype(f32)
        v = _rotate(_conj(rot), np.broadcast_to(ray["dir"].astype(f32), (n, 3)), f32) * inv  # invTransformVector, :789-797
        inv_len = f32(1) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])  # normalize, :367-376
        d = v * inv_len[:, None]
        # getRaySphereIntersection(o, d, ZERO, radius, t) && t >= 0
        L = f32(0) - o
        tca = _dot(L, d)
        d2 = _dot(L, L) - tca * tca
        rr = radius * radius
        thc = np.sqrt(rr - d2)
        t = tca - thc
        out = np.where(t >= 0, t, tca + thc)
        sphere = ~(d2 > rr) & (out >= 0)
        # getRayAABBIntersection(o, d, aabb.min, aabb.max - aabb.min)
        mn = models["aabb_min"][m].astype(f32)
        mx = mn + (models["aabb_max"][m].astype(f32) - mn)
        frac = f32(1) / np.where(d == 0, f32(0.00000001), d)
        lo, hi = (mn - o) * frac, (mx - o) * frac
        tmin = _maximum(_maximum(_minimum(lo[:, 0], hi[:, 0]), _minimum(lo[:, 1], hi[:, 1])), _minimum(lo[:, 2], hi[:, 2]))
        tmax = _minimum(_minimum(_maximum(lo[:, 0], hi[:, 0]), _maximum(lo[:, 1], hi[:, 1])), _maximum(lo[:, 2], hi[:, 2]))
        aabb = ~(tmax < 0) & ~(tmin > tmax)
    return has & sphere & aabb, gate, o, d


def _skin(positions, skin, mats):
    """evaluateSkin for every vertex: ((M0 w.x + M1 w.y) + M2 w.z) + M3 w.w element by element, then Matrix::transformPoint."""
    idx = skin["indices"].astype(np.int64) & 0xffff
    idx = np.where(idx < len(mats), idx, 0)
    w = skin["weights"].astype(f32)
    m = mats[idx[:, 0]] * w[:, 0, None, None]
    for k in (1, 2, 3):
        m = m + mats[idx[:, k]] * w[:, k, None, None]
    p = positions
    return np.stack([m[:, 0, r] * p[:, 0] + m[:, 1, r] * p[:, 1] + m[:, 2, r] * p[:, 2] + m[:, 3, r] for r in range(3)], -1)


def _corners(scene, model_index, entity):
    """(p0, p1, p2, mesh of each triangle) of the model's LOD 0 as Model::castRay sees it for this entity, cached."""
    mo = scene["models"][model_index]
    meshes = scene["meshes"][int(mo["first_mesh"]) : int(mo["first_mesh"]) + int(mo["mesh_count"])]
    mats = scene.get("palettes", {}).get(entity)
    # is_skinned = the verdict of the LAST mesh (model.cpp:147-150)
    is_skinned = bool(meshes) and mats is not None and meshes[-1]["skin"] is not None and len(mats) <= 256
    cache = scene.setdefault("_corners", {})
    key = (model_index, entity if is_skinned else -1)
    if key not in cache:
        ps, of = [], []
        for k, me in enumerate(meshes):
            v = np.asarray(me["positions"], f32).reshape(-1, 3)
            if is_skinned and me["skin"] is not None:
                with np.errstate(all="ignore"):
                    v = _skin(v, me["skin"], np.asarray(mats, f32))
            tri = np.asarray(me["indices"]).astype(np.int64).reshape(-1, 3)
            ps.append(v[tri])
            of.append(np.full(len(tri), k, np.int64))
        p = np.concatenate(ps) if ps else np.zeros((0, 3, 3), f32)
        cache[key] = (p[:, 0], p[:, 1], p[:, 2], np.concatenate(of) if of else np.zeros(0, np.int64))
    return cache[key]


def _narrow(scene, model_index, entity, o, d, nan_is_hit):
    """Model::castRay -> (t, mesh relative to LOD 0's first, triangle within the mesh) or None."""
    p0, p1, p2, mesh_of = _corners(scene, model_index, entity)
    if len(p0) == 0:
        return None
    with np.errstate(all="ignore"):
        normal = _cross(p1 - p0, p2 - p0)
        q = _dot(normal, d)
        dd = -_dot(normal, p0)
        t = -(_dot(normal, o) + dd) / q
        hp = o + d * t[:, None]
        ok = ~(q == 0) & ~(t < 0)
        ok &= ~(_dot(normal, _cross(p1 - p0, hp - p0)) < 0)
        ok &= ~(_dot(normal, _cross(p2 - p1, hp - p1)) < 0)
        ok &= ~(_dot(normal, _cross(p0 - p2, hp - p2)) < 0)
    if nan_is_hit and np.isnan(t[ok]).any():  # `!hit.is_hit || hit.t > t` one triangle after the other: a NaN that comes first stays
        best = -1
        for i in np.flatnonzero(ok):
            if best < 0 or t[best] > t[i]:
                best = i
    else:
        ok &= ~np.isnan(t)
        if not ok.any():
            return None
        best = int(np.argmin(np.where(ok, t, f32(np.inf))))  # the first of the smallest (-0 == +0)
        if not ok[best]:
            best = int(np.flatnonzero(ok)[0])  # every t is +inf
    first = int(np.flatnonzero(mesh_of == mesh_of[best])[0])
    return f32(t[best]), int(mesh_of[best]), int(best - first)


def _new_t(ray, pos, rot, scale, o, d, t):
    """:2743-2745 with hit.origin = DVec3(origin) of model.cpp:220"""
    with np.errstate(all="ignore"):
        p = (o.astype(f64) + (d * t).astype(f64)).astype(f32)
        world = pos + _rotate(rot, p * scale, f32).astype(f64)  # Transform::transform(Vec3), core/math.cpp:765
        dp = ray["origin"].astype(f64) - world
        return f32(np.sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]))


def _cast(scene, rays, sequential):
    rays = np.asarray(rays)
    out = np.zeros(len(rays), HIT)
    tr = _transforms(scene, len(scene["inst_model"]))
    models = scene["models"]
    for r, ray in enumerate(rays):
        passes, gate, o, d = _broad(scene, ray, tr)
        cur_dist = f64(ray["t_max"])  # +inf stands for DBL_MAX
        hit_t = f32(ray["t_max"])
        for e in np.flatnonzero(passes):
            if gate[e] > cur_dist:
                continue
            mi = int(scene["inst_model"][e])
            got = _narrow(scene, mi, int(e), o[e], d[e], nan_is_hit=sequential)
            if got is None:
                continue
            t, mesh, tri = got
            new_t = _new_t(ray, tr[0][e], tr[1][e], tr[2][e], o[e], d[e], t)
            if new_t < hit_t:  # (`!hit.is_hit || new_t < hit.t` with hit.t = t_max before the first hit)
                out[r] = (1, e, int(models[mi]["lod0_from"]) + mesh, tri, new_t, t)
                hit_t = new_t
                if sequential:
                    cur_dist = f64(new_t)
    return out


def cast_sequential(scene, rays):
    return _cast(scene, rays, True)


def cast(scene, rays):
    return _cast(scene, rays, False)


def agrees(scene, rays) -> bool:
    return cast(scene, rays).tobytes() == cast_sequential(scene, rays).tobytes()


def candidates(scene, rays) -> int:
    """(ray, entity) pairs that pass steps 1-6 against t_max: what the device counts"""
    tr = _transforms(scene, len(scene["inst_model"]))
    n = 0
    for ray in np.asarray(rays):
        passes, gate, _, _ = _broad(scene, ray, tr)
        n += int((passes & ~(gate > f64(ray["t_max"]))).sum())
    return n
