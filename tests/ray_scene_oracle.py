"""numpy restatement of the rest of RenderModuleImpl::castRay behind the model-instance loop: castRayProceduralGeometry
(renderer/render_module.cpp:2650-2712), Terrain::castRay with both Terrain::getHeight (renderer/terrain.cpp:402-447, 474-535),
getRayAABBIntersection / getRayTriangleIntersection / AABB::contains (core/geometry.cpp) and the merge of :2761-2775, built on
tests/ray_oracle.py and tests/ray_im_oracle.py.

Written from the description of the algorithm, line by line cited, with none of the reference's text. Every product, sum and quotient is
one np.float32 step in the reference's order (numpy never fuses); the fp64 steps are `ray.origin - pos` and Transform::invTransform. Forms:

  cast_pg_sequential  the reference's walk: geometries in table order, triangles in order, a later triangle replaces the hit when its t is
                      strictly smaller; a NaN t that comes first stays;
  cast_pg             the order-free form the device computes: the smallest t over every castable geometry, ties to the smallest
                      (geometry, triangle), -0 == +0, a NaN t is no hit. Neither form looks at t_max;
  agrees_pg           both give the same hits: a scene for the device tests must make it true;
  cast_terrain        -> (hits[ray, terrain], walk_ends[ray, terrain]): the first cell along the walk with a hit and the first triangle of
                      that cell; walk_ends is False where the reference's loop would never return (a zero step in the chosen branch: the
                      device ends such a walk without a hit, and so does this function);
  cast_scene          -> {"im", "hits", "pg", "terrain", "scene"}: every stage's records and castRay's result;
  candidates_pg       (ray, geometry) pairs that pass the gate: what the device counts;
  agrees              every stage gives the same hits in its walk-order and order-free forms.

A scene is ray_im_oracle's dict plus
  pg        list of {"entity", "aabb_min", "aabb_max", "vertex_data" (any array: its bytes), "stride", "indices" (None / uint16 / uint32),
                     optional "index_count", "triangles" (default True)} in m_procedural_geometries.iterated() order
  terrains  list of {"entity", "scale" (x, y, z), "heightmap" ((height, width) uint16: R16, uint32: RGBA8), "ready" (default True)} in
            m_terrains order
"""
import numpy as np

from tests import ray_im_oracle as RIO
from tests import ray_oracle as RO
from tests.ray_oracle import _conj, _cross, _dot, _maximum, _minimum, _rotate, _safe_inv, f32, f64

PG_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("geom", "<u4"), ("triangle", "<u4"), ("t", "<f4")])
TERRAIN_HIT = np.dtype([("is_hit", "<u4"), ("entity", "<i4"), ("terrain", "<u4"), ("hx", "<i4"), ("hz", "<i4"), ("tri", "<u4"), ("t", "<f4")])
SCENE_HIT = np.dtype([("is_hit", "<u4"), ("component", "<u4"), ("entity", "<i4"), ("index", "<u4"), ("sub", "<u4"), ("t", "<f4")])
MODEL_INSTANCE, INSTANCED_MODEL, PROCEDURAL_GEOM, TERRAIN = 1, 2, 3, 4


def _transform_of(scene, e):
    tr = scene["transforms"]
    if 0 <= e < len(tr):
        return tr["pos"][e].astype(f64), tr["rot"][e].astype(f32), tr["scale"][e].astype(f32)
    return np.zeros(3, f64), np.zeros(4, f32), np.zeros(3, f32)  # an entity the table does not cover reads as zero


def _refused(ray, entity):  # the filter of castRay(ray, ignored), :2603-2607
    return int(ray["ignore"]) >= 0 and int(entity) == int(ray["ignore"])


# ---- procedural geometry ----------------------------------------------------------------------------------------------------------
def _pg_corners(g):
    """(p0, p1, p2) of every triangle the reference walks, or None when the geometry is never cast (:2655-2656, :2672-2699)"""
    if "_corners" not in g:
        data = np.frombuffer(np.ascontiguousarray(g["vertex_data"]).tobytes(), np.uint8)
        g["_corners"] = None
        if len(data) and g.get("triangles", True):
            stride = int(g["stride"])
            n_verts = len(data) // stride
            pos = np.stack([np.frombuffer(data[v * stride : v * stride + 12].tobytes(), f32) for v in range(n_verts)]) if n_verts else np.zeros((0, 3), f32)
            idx = g.get("indices")
            if idx is not None and len(idx):
                idx = np.asarray(idx).reshape(-1).astype(np.int64)
                n_tris = int(g.get("index_count", len(idx))) // 3
            else:
                n_tris = n_verts // 3
                idx = np.arange(3 * n_tris, dtype=np.int64)
            p = pos[idx[: 3 * n_tris].reshape(-1, 3)] if n_tris else np.zeros((0, 3, 3), f32)
            g["_corners"] = (p[:, 0], p[:, 1], p[:, 2])
    return g["_corners"]


def _pg_ray(scene, g, ray):
    """:2663-2666 -> (ro, rd): rd is NOT normalised"""
    pos, rot, scale = _transform_of(scene, int(g["entity"]))
    with np.errstate(all="ignore"):
        inv = _safe_inv(scale)
        rd = _rotate(_conj(rot), ray["dir"].astype(f32), f32) * inv  # invTransformVector, core/math.cpp:789-797
        rotated = _rotate(_conj(rot), ray["origin"].astype(f64) - pos, f64)  # invTransform(DVec3), core/math.cpp:767-774
        ro = (rotated * inv.astype(f64)).astype(f32)
    return ro, rd


def _ray_aabb(o, d, mn, size):
    """getRayAABBIntersection, core/geometry.cpp:861-889 -> (hit, tmin)"""
    with np.errstate(all="ignore"):
        frac = f32(1) / np.where(d == 0, f32(0.00000001), d).astype(f32)
        mx = (mn + size).astype(f32)
        lo, hi = (mn - o) * frac, (mx - o) * frac
        tmin = _maximum(_maximum(_minimum(lo[0], hi[0]), _minimum(lo[1], hi[1])), _minimum(lo[2], hi[2]))
        tmax = _minimum(_minimum(_maximum(lo[0], hi[0]), _maximum(lo[1], hi[1])), _maximum(lo[2], hi[2]))
        return bool(~(tmax < 0) & ~(tmin > tmax)), f32(tmin)


def _pg_gate(g, ro, rd):
    """`aabb.contains(ro) || getRayAABBIntersection(ro, rd, aabb.min, aabb.max - aabb.min)`, :2669; AABB::contains core/geometry.cpp:540-548"""
    mn, mx = np.asarray(g["aabb_min"], f32), np.asarray(g["aabb_max"], f32)
    if not ((mn > ro).any() or (ro > mx).any()):
        return True
    return _ray_aabb(ro, rd, mn, (mx - mn).astype(f32))[0]


def _triangles(p0, p1, p2, o, d):
    """getRayTriangleIntersection for many triangles, core/geometry.cpp:927-967 -> (returns true, t)"""
    with np.errstate(all="ignore"):
        normal = _cross(p1 - p0, p2 - p0)
        q = _dot(normal, d)
        dd = -_dot(normal, p0)
        t = -(_dot(normal, o) + dd) / q
        hp = o + d * t[..., None]
        ok = ~(q == 0) & ~(t < 0)
        ok &= ~(_dot(normal, _cross(p1 - p0, hp - p0)) < 0)
        ok &= ~(_dot(normal, _cross(p2 - p1, hp - p1)) < 0)
        ok &= ~(_dot(normal, _cross(p0 - p2, hp - p2)) < 0)
    return ok, t.astype(f32)


def _pg_walk(scene, ray):
    """per castable geometry that passes its gate, in table order: (index, entity, ok[tri], t[tri])"""
    for k, g in enumerate(scene.get("pg", [])):
        corners = _pg_corners(g)
        if corners is None or _refused(ray, g["entity"]):  # (the filter refuses every one of its triangles, :2703-2705)
            continue
        ro, rd = _pg_ray(scene, g, ray)
        if not _pg_gate(g, ro, rd):
            continue
        ok, t = _triangles(*corners, ro, rd) if len(corners[0]) else (np.zeros(0, bool), np.zeros(0, f32))
        yield k, int(g["entity"]), ok, t


def cast_pg_sequential(scene, rays):
    rays = np.asarray(rays)
    out = np.zeros(len(rays), PG_HIT)
    for r, ray in enumerate(rays):
        hit = None
        for k, entity, ok, t in _pg_walk(scene, ray):
            for i in np.flatnonzero(ok):
                if hit is None or t[i] < hit[4]:  # `t < hit.t || !hit.is_hit`, :2700
                    hit = (1, entity, k, int(i), t[i])
        if hit is not None:
            out[r] = hit
    return out


def cast_pg(scene, rays):
    rays = np.asarray(rays)
    out = np.zeros(len(rays), PG_HIT)
    for r, ray in enumerate(rays):
        hit = None
        for k, entity, ok, t in _pg_walk(scene, ray):
            ok = ok & ~np.isnan(t)
            if not ok.any():
                continue
            i = int(np.argmin(np.where(ok, t, f32(np.inf))))  # the first of the smallest (-0 == +0)
            if not ok[i]:
                i = int(np.flatnonzero(ok)[0])  # every t is +inf
            if hit is None or t[i] < hit[4]:  # (table order: a tie keeps the earlier geometry)
                hit = (1, entity, k, i, t[i])
        if hit is not None:
            out[r] = hit
    return out


def agrees_pg(scene, rays) -> bool:
    return cast_pg(scene, rays).tobytes() == cast_pg_sequential(scene, rays).tobytes()


def candidates_pg(scene, rays) -> int:
    return sum(1 for ray in np.asarray(rays) for _ in _pg_walk(scene, ray))


# ---- terrain ----------------------------------------------------------------------------------------------------------------------
def _trunc(v):
    """(int)v as x86's cvttss2si gives it: NaN and values outside int32 are INT32_MIN"""
    v = float(v)
    return int(v) if -2147483648.0 <= v < 2147483648.0 else -(1 << 31)


def _clamp(v, lo, hi):  # core/math.h:520-522: minimum(maximum(value, min), max)
    m = v if v > lo else lo
    return m if m < hi else hi


class _Terrain:
    def __init__(self, t):
        self.map = np.ascontiguousarray(t["heightmap"])
        self.h, self.w = self.map.shape
        self.r16 = self.map.dtype == np.uint16
        self.sx, self.sy, self.sz = (f32(v) for v in t["scale"])
        self.entity = int(t["entity"])
        self.ready = bool(t.get("ready", True))

    def texel_height(self, x, z):  # Terrain::getHeight(int, int), :430-447: scale.y * DIV * texel, left to right
        texel = int(self.map[_clamp(z, 0, self.h - 1), _clamp(x, 0, self.w - 1)])
        if self.r16:
            return self.sy * (f32(1) / f32(65535)) * f32(texel)
        return self.sy * (f32(1) / f32(255)) * f32(texel & 0xff)

    def height(self, x, z):  # Terrain::getHeight(float, float), :402-427
        inv_scale = f32(1) / self.sx
        ix, iz = _trunc(x * inv_scale), _trunc(z * inv_scale)
        dec_x = (x - f32(ix) * self.sx) * inv_scale
        dec_z = (z - f32(iz) * self.sx) * inv_scale
        if dec_z == 0 and dec_x == 0:
            return self.texel_height(ix, iz)
        if dec_x > dec_z:
            h0, h1, h2 = self.texel_height(ix, iz), self.texel_height(ix + 1, iz), self.texel_height(ix + 1, iz + 1)
            return h0 + (h1 - h0) * dec_x + (h2 - h1) * dec_z
        h0, h1, h2 = self.texel_height(ix, iz), self.texel_height(ix + 1, iz + 1), self.texel_height(ix, iz + 1)
        return h0 + (h2 - h0) * dec_z + (h1 - h2) * dec_x

    def cast(self, pos, ray):
        """-> ((hx, hz, tri, t, iteration of the walk) or None, walk_ends)"""
        if not self.ready:
            return None, True
        with np.errstate(all="ignore"):
            rel = (ray["origin"].astype(f64) - pos).astype(f32)  # Vec3(ray.origin - pos), :483
            d = ray["dir"].astype(f32)
            size = np.array([f32(self.w) * self.sx, self.sy * f32(65535.0), f32(self.h) * self.sx], f32)
            ok, tmin = _ray_aabb(rel, d, np.zeros(3, f32), size)
            if not ok:
                return None, True
            start = rel if tmin < 0 else rel + d * tmin
            hx, hz = _trunc(start[0] / self.sx), _trunc(start[2] / self.sx)
            flat_x, flat_z = abs(d[0]) < f32(0.01), abs(d[2]) < f32(0.01)
            next_x = f32(hx) if flat_x else (f32(hx + (0 if d[0] < 0 else 1)) * self.sx - rel[0]) / d[0]
            next_z = f32(hz) if flat_z else (f32(hz + (0 if d[2] < 0 else 1)) * self.sx - rel[2]) / d[2]
            delta_x = f32(0) if flat_x else self.sx / abs(d[0])
            delta_z = f32(0) if flat_z else self.sz / abs(d[2])  # (scale.z, :496)
            step_x = 1 if d[0] > 0 else (-1 if d[0] < 0 else 0)
            step_z = 1 if d[2] > 0 else (-1 if d[2] < 0 else 0)
            for step in range(self.w + self.h):  # a walk that ends moves hx or hz by one per iteration
                if not (hx >= 0 and hz >= 0 and hx + step_x < self.w and hz + step_z < self.h):
                    return None, True
                x, z = f32(hx) * self.sx, f32(hz) * self.sx
                x1, z1 = x + self.sx, z + self.sx
                p = [np.array(c, f32) for c in ((x, self.height(x, z), z), (x1, self.height(x1, z), z), (x1, self.height(x1, z1), z1), (x, self.height(x, z1), z1))]
                for tri, (a, b, c) in enumerate(((p[0], p[1], p[2]), (p[0], p[2], p[3]))):
                    hit, t = _triangles(a, b, c, rel, d)
                    if hit and not np.isnan(t):  # (a NaN t is no hit on the device, as in the other stages)
                        return (hx, hz, tri, f32(t), step), True
                if next_x < next_z and step_x != 0:
                    next_x = next_x + delta_x
                    hx += step_x
                else:
                    if step_z == 0 and not (delta_x == 0 and delta_z == 0):
                        return None, False  # nothing changes from here on: the reference never returns
                    next_z = next_z + delta_z
                    hz += step_z
                if delta_x == 0 and delta_z == 0:
                    return None, True
        return None, True


def cast_terrain(scene, rays, steps=None):
    """steps: an int array [ray, terrain] that receives the iteration of the walk a hit was found in (-1: none)"""
    rays = np.asarray(rays)
    terrains = [_Terrain(t) for t in scene.get("terrains", [])]
    out = np.zeros((len(rays), len(terrains)), TERRAIN_HIT)
    ends = np.ones((len(rays), len(terrains)), bool)
    for k, te in enumerate(terrains):
        pos = _transform_of(scene, te.entity)[0]  # world.getPosition(m_entity), :482
        for r, ray in enumerate(rays):
            got, ends[r, k] = te.cast(pos, ray)
            if steps is not None:
                steps[r, k] = -1 if got is None else got[4]
            if got is not None:
                out[r, k] = (1, te.entity, k, got[0], got[1], got[2], got[3])
    return out, ends


# ---- castRay ----------------------------------------------------------------------------------------------------------------------
def merge(scene, rays, im_hits, hits, pg_hits, terrain_hits):
    """:2718-2775 over the stages' records"""
    rays = np.asarray(rays)
    out = np.zeros(len(rays), SCENE_HIT)
    widths = [np.asarray(t["heightmap"]).shape[1] for t in scene.get("terrains", [])]
    for r, ray in enumerate(rays):
        hit = None
        if hits[r]["is_hit"]:
            hit = (1, MODEL_INSTANCE, hits[r]["entity"], hits[r]["mesh"], hits[r]["triangle"], hits[r]["t"])
        elif im_hits is not None and im_hits[r]["is_hit"]:
            hit = (1, INSTANCED_MODEL, im_hits[r]["entity"], im_hits[r]["model"], im_hits[r]["subindex"], im_hits[r]["t"])
        pg = pg_hits[r]
        if pg["is_hit"] and pg["t"] < ray["t_max"] and (hit is None or pg["t"] < hit[5]):  # :2762, below the hit the caller holds
            hit = (1, PROCEDURAL_GEOM, pg["entity"], pg["geom"], pg["triangle"], pg["t"])
        for k in range(terrain_hits.shape[1]):  # :2767-2775
            th = terrain_hits[r, k]
            if th["is_hit"] and th["t"] < ray["t_max"] and (hit is None or th["t"] < hit[5]) and not _refused(ray, th["entity"]):
                hit = (1, TERRAIN, th["entity"], k, int(th["hz"]) * widths[k] + int(th["hx"]), th["t"])
        if hit is not None:
            out[r] = hit
    return out


def cast_scene(scene, rays):
    rays = np.asarray(rays)
    if scene.get("im_models") is not None:
        im_hits, hits = RIO.cast_all(scene, rays)
    else:
        im_hits, hits = None, RO.cast(scene, rays)
    pg_hits = cast_pg(scene, rays)
    terrain_hits, ends = cast_terrain(scene, rays)
    return {"im": im_hits, "hits": hits, "pg": pg_hits, "terrain": terrain_hits, "walk_ends": ends, "scene": merge(scene, rays, im_hits, hits, pg_hits, terrain_hits)}


def agrees(scene, rays) -> bool:
    rays = np.asarray(rays)
    first = RIO.agrees(scene, rays) if scene.get("im_models") is not None else RO.agrees(scene, rays)
    return first and agrees_pg(scene, rays)
