"""numpy restatement of RenderModuleImpl::castRayInstancedModels (renderer/render_module.cpp:2609-2648) and of how castRay joins its
result with the model-instance loop (:2718-2719, :2746), built on tests/ray_oracle.py (Model::castRay, the sphere test, Quat::rotate).

Written from the description of the algorithm, line by line cited, with none of the reference's text. Every product, sum, quotient and
root is one np.float32 step in the reference's order; the one fp64 step is `ray.origin - tr.pos`. Forms:

  cast_im_sequential  the reference's walk: models in registration order, instances in stored order, the first hit stays unless a later
                      t_model * scale is strictly smaller; a NaN that comes first stays (as in Model::castRay). The caller's `held` rule
                      is applied to its result: the hit counts when its t < ray.t_max;
  cast_im             the order-free form the device computes: per ray the smallest t_model * scale below t_max over every instance of
                      every model (ties: the smallest model, then the smallest stored index; -0 == +0), a NaN is no hit;
  cast_all            (instanced-model hits, model-instance hits): the second under the effective t_max - the instanced-model hit's t
                      where there is one (`cur_dist`, `new_t < hit.t`), else the ray's own;
  candidates_im       (ray, instance) pairs that pass the sphere: what the device counts;
  agrees              both stages give the same hits in both forms: a scene for the device tests must make it true.

A scene is ray_oracle's dict plus
  im_models  list of {"ray_model": index into `models` (-1: none), "entity": int, "origin": (3,) f64 - World::getTransform(e).pos,
                      "radius": f32 - Model::getOriginBoundingRadius, "instances": api.IM_INSTANCE array in STORED order}
"""
import numpy as np

from tests import ray_oracle as RO
from tests.ray_oracle import _conj, _dot, _narrow, _rotate, f32, f64

IM_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("model", "<u4"), ("subindex", "<u4"), ("mesh", "<u4"), ("triangle", "<u4"), ("t", "<f4"), ("t_model", "<f4")])


def _castable(scene, mdl, ray):
    """`!im.model || !isReady()` (:2616); the `ignore` filter (:2603-2607) refuses every triangle of a model whose entity it names"""
    rm = int(mdl["ray_model"])
    if rm < 0 or rm >= len(scene["models"]) or scene["models"][rm]["ready"] == 0:
        return False
    return int(mdl["entity"]) != int(ray["ignore"])


def _instances(mdl, ray):
    """:2628-2634 for every instance of a model at once -> (passes the sphere, rel_pos, rel_dir, scale)"""
    inst = mdl["instances"]
    n = len(inst)
    with np.errstate(all="ignore"):
        base = (ray["origin"].astype(f64) - np.asarray(mdl["origin"], f64)).astype(f32)  # Vec3(ray.origin - tr.pos)
        scale = inst["scale"].astype(f32)
        rel = base[None, :] - inst["pos"].astype(f32)
        radius = f32(mdl["radius"]) * scale
        d = np.broadcast_to(ray["dir"].astype(f32), (n, 3))
        # getRaySphereIntersection(rel, dir, ZERO, radius, t) && t >= 0, core/geometry.cpp:844-859
        L = f32(0) - rel
        tca = _dot(L, d)
        d2 = _dot(L, L) - tca * tca
        rr = radius * radius
        thc = np.sqrt(rr - d2)
        t = tca - thc
        out = np.where(t >= 0, t, tca + thc)
        sphere = ~(d2 > rr) & (out >= 0)
        q = inst["rot"].astype(f32)
        w = np.sqrt(f32(1) - (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]))  # getInstanceQuat, :2619-2626
        rot = np.concatenate([q, w[:, None]], 1).astype(f32)
        rel_dir = _rotate(_conj(rot), d, f32)
        tmp = f32(1) / scale  # Vec3::operator/(float), core/math.cpp:471-474
        rel_pos = _rotate(_conj(rot), rel * tmp[:, None], f32)
    return sphere, rel_pos, rel_dir, scale


def _walk(scene, ray, sequential):
    """every (model, stored index, mesh, triangle, t_model, t_model * scale) with a triangle hit, in the reference's order"""
    for m, mdl in enumerate(scene.get("im_models", [])):
        if not _castable(scene, mdl, ray) or len(mdl["instances"]) == 0:
            continue
        sphere, rel_pos, rel_dir, scale = _instances(mdl, ray)
        rm = int(mdl["ray_model"])
        for i in np.flatnonzero(sphere):
            got = _narrow(scene, rm, -1, rel_pos[i], rel_dir[i], nan_is_hit=sequential)  # pose == nullptr: never skinned
            if got is None:
                continue
            t, mesh, tri = got
            with np.errstate(all="ignore"):
                yield m, int(i), int(scene["models"][rm]["lod0_from"]) + mesh, tri, t, f32(t * scale[i])


def _record(scene, m, i, mesh, tri, t, prod):
    return (1, int(scene["im_models"][m]["entity"]), m, i, mesh, tri, prod, t)


def cast_im_sequential(scene, rays):
    rays = np.asarray(rays)
    out = np.zeros(len(rays), IM_HIT)
    for r, ray in enumerate(rays):
        hit = None
        for m, i, mesh, tri, t, prod in _walk(scene, ray, True):
            if hit is None or prod < hit[6]:  # `!hit.is_hit || new_hit.t * id.scale < hit.t`, :2636
                hit = _record(scene, m, i, mesh, tri, t, prod)
        if hit is not None and hit[6] < f32(ray["t_max"]):  # the caller's `held`
            out[r] = hit
    return out


def cast_im(scene, rays):
    rays = np.asarray(rays)
    out = np.zeros(len(rays), IM_HIT)
    for r, ray in enumerate(rays):
        hit = None
        for m, i, mesh, tri, t, prod in _walk(scene, ray, False):
            if not prod < f32(ray["t_max"]):  # (a NaN is below nothing)
                continue
            if hit is None or prod < hit[6]:  # (the walk is in (model, stored index) order: a tie keeps the earlier)
                hit = _record(scene, m, i, mesh, tri, t, prod)
        if hit is not None:
            out[r] = hit
    return out


def effective_rays(rays, im_hits):
    """the rays as the model-instance loop sees them: t_max = the instanced-model hit's t where there is one"""
    eff = np.array(rays, copy=True)
    got = im_hits["is_hit"] == 1
    eff["t_max"][got] = im_hits["t"][got]
    return eff


def cast_all(scene, rays):
    im_hits = cast_im(scene, rays)
    return im_hits, RO.cast(scene, effective_rays(rays, im_hits))


def candidates_im(scene, rays) -> int:
    n = 0
    for ray in np.asarray(rays):
        for mdl in scene.get("im_models", []):
            if _castable(scene, mdl, ray) and len(mdl["instances"]):
                n += int(_instances(mdl, ray)[0].sum())
    return n


def agrees(scene, rays) -> bool:
    a, b = cast_im(scene, rays), cast_im_sequential(scene, rays)
    return a.tobytes() == b.tobytes() and RO.agrees(scene, effective_rays(rays, a))
