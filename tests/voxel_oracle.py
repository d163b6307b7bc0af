"""Voxels of renderer/voxels.cpp restated in numpy: the checker of the voxel kernels and of lmx_voxels_grid / _rng_skip.

Every float is an np.float32 and every operation one IEEE operation in the reference's order; numpy neither fuses nor reassociates. The
generator is stepped sequentially - that is its reference form here; the product's closed-form skip is checked against it. Loops over
cells and rays are array operations, which changes no value: a voxel set has no order, and a ray depends on its three draws alone.

tests/test_voxel_oracle_vs_ref.py holds this file to the reference's own code, and settles that g++ evaluates the arguments of
`Vec3(randFloat(), randFloat(), randFloat())` right to left: the first draw is z.

RULES names the one-rule mutants of tests/test_voxels_cpu.py: Voxels(rule=True) changes exactly that rule.
"""
import numpy as np

F = np.float32
INT_MIN = -(2 ** 31)
RULES = ("draw_order_reversed", "true_division", "floor", "one_step", "inclusive_bounds", "blur_27", "ao_by_product", "aabb_all_vertices")


def f32(a):
    return np.asarray(a, dtype=np.float32)


def vmin(a, b):  # core/math.h minimum: a < b ? a : b
    return np.where(a < b, a, b)


def vmax(a, b):  # a > b ? a : b
    return np.where(a > b, a, b)


def vmin3(a, b, c):
    return vmin(a, vmin(b, c))


def vmax3(a, b, c):
    return vmax(a, vmax(b, c))


def i32(v, floor=False):
    """int(float) of x86-64: truncation; NaN and values outside the range give INT_MIN (the `floor` mutant rounds down instead)"""
    v = f32(v)
    with np.errstate(invalid="ignore"):
        ok = (v > F(-2147483904.0)) & (v < F(2147483648.0))
        r = np.floor(v) if floor else np.trunc(v)
        return np.where(ok, np.where(ok, r, 0).astype(np.int64), INT_MIN)


# ---- RandomGenerator (core/math.cpp:1337-1378) ----------------------------------------------------------------------------------------
def rng_step(u, v):
    u = (36969 * (u & 65535) + (u >> 16)) & 0xFFFFFFFF
    v = (18000 * (v & 65535) + (v >> 16)) & 0xFFFFFFFF
    return u, v


def rng_draws(u, v, n):
    """n values of rand() behind (u, v), stepped one by one -> (uint32 array, the state behind them)"""
    out = np.empty(n, np.uint32)
    for k in range(n):
        u, v = rng_step(u, v)
        out[k] = ((u << 16) + v) & 0xFFFFFFFF
    return out, (u, v)


def rng_skip_sequential(u, v, n):
    for _ in range(n):
        u, v = rng_step(u, v)
    return u, v


def rand_floats(draws):
    return (draws.astype(np.float64) * 2.328306435996595e-10).astype(np.float32)  # float(rand() * 2.328306435996595e-10)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def grid(aabb_min, aabb_max, max_res):
    """beginRaster (voxels.cpp:172-185) -> (min, max, voxel_size, resolution)"""
    mn, mx = f32(aabb_min).copy(), f32(aabb_max).copy()
    with np.errstate(all="ignore"):
        vs = vmax3(mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]) / F(max_res)
        vs = F(vs)
        mn = mn - vs * F(1.5)
        mx = mx + vs * F(1.5)
        res = i32((mx - mn) / vs)
    return mn, mx, vs, res.astype(np.int64)


def mesh_triangles(positions, indices):
    p = f32(positions)[:, :3]
    return p[np.asarray(indices, np.int64).reshape(-1, 3)]  # (n, 3 corners, 3)


class Voxels:
    def __init__(self, **rules):
        assert all(k in RULES for k in rules)
        self.rules = {k: bool(rules.get(k)) for k in RULES}
        self.ao = None
        self.rng = None

    # -- raster ---------------------------------------------------------------------------------------------------------------------------
    def beginRaster(self, aabb_min, aabb_max, max_res):
        self.mn, self.mx, self.vs, self.res = grid(aabb_min, aabb_max, max_res)
        self.voxels = np.zeros(int(self.res[0] * self.res[1] * self.res[2]), np.uint8)

    def info(self):
        return self.mn, self.mx, self.vs, self.res

    def to_grid(self, p):
        if self.rules["true_division"]:
            q = (f32(p) - self.mn) / self.vs + F(0.5)
        else:
            tmp = F(1) / self.vs  # Vec3::operator/(float)
            q = (f32(p) - self.mn) * tmp + F(0.5)
        return i32(q, self.rules["floor"])

    def raster(self, positions, indices):
        for tri in mesh_triangles(positions, indices):
            self.raster_triangle(tri[0], tri[1], tri[2])

    def raster_triangle(self, p0, p1, p2):
        mn, mx = p0, p0
        mn, mx = vmin(p1, mn), vmax(p1, mx)  # AABB::addPoint
        mn, mx = vmin(p2, mn), vmax(p2, mx)
        lo = np.maximum(self.to_grid(mn - self.vs), 0)
        hi = np.minimum(self.to_grid(mx), self.res - 1)  # setVoxel skips the cells outside the grid
        if np.any(hi < lo):
            return
        k, j, i = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
        i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
        hit = self.cell_hits_triangle(i, j, k, p0, p1, p2)
        self.voxels[(i + (j + k * self.res[1]) * self.res[0])[hit]] = 1

    def cell_hits_triangle(self, i, j, k, a, b, c):
        """testAABBTriangleCollision (core/geometry.cpp:1007-1066) on raster's box of a cell, for arrays of cells"""
        vs = self.vs
        hv = F(0.5) * vs
        with np.errstate(all="ignore"):
            center = [f32(i) * vs + hv + self.mn[0], f32(j) * vs + hv + self.mn[1], f32(k) * vs + hv + self.mn[2]]  # from_grid
            bmin = [cc - hv for cc in center]
            bmax = [cc + hv for cc in center]
            ac = [(bmax[n] + bmin[n]) * F(0.5) for n in range(3)]
            half = [(bmax[n] - bmin[n]) * F(0.5) for n in range(3)]
            v1 = [a[n] - ac[n] for n in range(3)]
            v2 = [b[n] - ac[n] for n in range(3)]
            v3 = [c[n] - ac[n] for n in range(3)]
            sub = lambda p, q: [p[n] - q[n] for n in range(3)]
            cross = lambda p, q: [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
            dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
            us = ([F(1), F(0), F(0)], [F(0), F(1), F(0)], [F(0), F(0), F(1)])
            es = (sub(v2, v1), sub(v3, v2), sub(v1, v3))
            ok = np.ones(len(i), bool)
            for u in us:
                for e in es:
                    n = cross(u, e)
                    p0, p1, p2 = dot(v1, n), dot(v2, n), dot(v3, n)
                    r = dot(half, [np.abs(n[0]), np.abs(n[1]), np.abs(n[2])])
                    ok &= ~(vmax(-vmax3(p0, p1, p2), vmin3(p0, p1, p2)) > r)
            for n in range(3):
                lo, hi = vmin3(v1[n], v2[n], v3[n]), vmax3(v1[n], v2[n], v3[n])
                ok &= ~((lo > half[n]) | (hi < -half[n]))
            normal = cross(es[0], es[1])
            d = dot(normal, v1)
            vm = [np.where(normal[n] > F(0), -half[n], half[n]) for n in range(3)]
            ok &= ~(dot(normal, vm) > d)
            ok &= -dot(normal, vm) >= d
        return ok

    def voxelize(self, meshes, max_res):
        """voxelize(Model&, max_res) (voxels.cpp:230-258): meshes = [(positions, indices)]; the AABB in index order"""
        mn, mx = f32([np.finfo(np.float32).max] * 3), f32([-np.finfo(np.float32).max] * 3)
        for positions, indices in meshes:
            pts = f32(positions)[:, :3] if self.rules["aabb_all_vertices"] else mesh_triangles(positions, indices).reshape(-1, 3)
            for p in pts:
                mn = vmin(mn, p)
                mx = vmax(mx, p)
        self.beginRaster(mn, mx, max_res)
        for positions, indices in meshes:
            self.raster(positions, indices)

    # -- ambient occlusion ----------------------------------------------------------------------------------------------------------------
    def computeAO(self, ray_count, u, v):
        """computeAO(ray_count) (voxels.cpp:122-141) with the generator at (u, v); self.rng = the generator behind it"""
        rx, ry, rz = (int(r) for r in self.res)
        n = rx * ry * rz
        draws, self.rng = rng_draws(u, v, 3 * ray_count * n)
        r = rand_floats(draws).reshape(n * ray_count, 3)
        if self.rules["draw_order_reversed"]:
            d = [r[:, 0], r[:, 1], r[:, 2]]
        else:
            d = [r[:, 2], r[:, 1], r[:, 0]]  # the first draw is z
        with np.errstate(all="ignore"):
            d = [c * F(2) - F(1) for c in d]
            m = vmax3(np.abs(d[0]), np.abs(d[1]), np.abs(d[2]))
            if self.rules["true_division"]:
                d = [c / m for c in d]
            else:
                inv = F(1) / m  # operator/= is *= 1.0f / rhs
                d = [c * inv for c in d]
            cell = np.repeat(np.arange(n, dtype=np.int64), ray_count)
            p = [f32(cell % rx) + F(0.5), f32(cell // rx % ry) + F(0.5), f32(cell // (rx * ry)) + F(0.5)]
            p = [p[k] + d[k] for k in range(3)]
            if not self.rules["one_step"]:
                p = [p[k] + d[k] for k in range(3)]  # castRay adds d again before its first sample
            s = [F(rx), F(ry), F(rz)]
            hit = np.zeros(n * ray_count, bool)
            live = np.ones(n * ray_count, bool)
            while True:
                if self.rules["inclusive_bounds"]:
                    inside = (p[0] >= 0) & (p[1] >= 0) & (p[2] >= 0) & (p[0] < s[0]) & (p[1] < s[1]) & (p[2] < s[2])
                else:
                    inside = (p[0] > 0) & (p[1] > 0) & (p[2] > 0) & (p[0] < s[0]) & (p[1] < s[1]) & (p[2] < s[2])
                live &= inside
                if not live.any():
                    break
                ip = [np.where(live, i32(np.where(live, c, 0), self.rules["floor"]), 0) for c in p]
                occ = self.voxels[ip[0] + (ip[1] + ip[2] * ry) * rx] != 0
                hit |= live & occ
                live &= ~occ
                p = [p[k] + d[k] for k in range(3)]
        hits = hit.reshape(n, ray_count).sum(axis=1)
        step = F(1) / F(ray_count)
        if self.rules["ao_by_product"]:
            self.ao = (F(1) - f32(hits) * step).astype(np.float32)
        else:
            table = np.empty(ray_count + 1, np.float32)  # `ao -= 1.f / ray_count` once per hit
            acc = F(1)
            for k in range(ray_count + 1):
                table[k] = acc
                acc = F(acc - step)
            self.ao = table[hits]

    def blurAO(self):
        rx, ry, rz = (int(r) for r in self.res)
        a3 = self.ao.reshape(rz, ry, rx)
        z, y, x = np.meshgrid(np.arange(rz), np.arange(ry), np.arange(rx), indexing="ij")
        v = np.zeros((rz, ry, rx), np.float32)
        for c in (-1, 0, 1):
            for b in (-1, 0, 1):
                for a in (-1, 0, 1):
                    v = v + a3[np.clip(z + c, 0, rz - 1), np.clip(y + b, 0, ry - 1), np.clip(x + a, 0, rx - 1)]
        self.ao = (v / F(27 if self.rules["blur_27"] else 9)).astype(np.float32).reshape(-1)

    # -- lookups --------------------------------------------------------------------------------------------------------------------------
    def point_cells(self, points):
        """sample / sampleAO's cell (voxels.cpp:49-57) -> (linear index, inside)"""
        p = f32(points).reshape(-1, 3)
        with np.errstate(all="ignore"):
            ip = i32((p - self.mn) / (self.mx - self.mn) * f32(self.res), self.rules["floor"])
        inside = np.all((ip >= 0) & (ip < self.res), axis=1)
        idx = np.where(inside, ip[:, 0] + (ip[:, 1] + ip[:, 2] * self.res[1]) * self.res[0], 0)
        return idx, inside

    def sample(self, points, fill=0xEE):
        idx, inside = self.point_cells(points)
        return np.where(inside, self.voxels[idx], fill).astype(np.uint8), inside.astype(np.uint8)

    def sampleAO(self, points, fill=-7.0):
        idx, inside = self.point_cells(points)
        return np.where(inside, self.ao[idx], F(fill)).astype(np.float32), inside.astype(np.uint8)

    def bakeVertexAO(self, points, min_ao, fill=0xEE):
        """model_importer.cpp:1339-1348: u8(clamp((ao + min_ao) * 255, 0.f, 255.f) + 0.5f); a vertex outside keeps its byte"""
        idx, inside = self.point_cells(points)
        with np.errstate(all="ignore"):
            v = (self.ao[idx] + F(min_ao)) * F(255)
            v = vmin(vmax(v, F(0)), F(255)) + F(0.5)
        return np.where(inside, np.trunc(v).astype(np.int64), fill).astype(np.uint8)


# ---- the cases of tests/test_gpu_voxels.py, tests/test_voxels_cpu.py and the recorded fixture -------------------------------------------
def box_mesh(lo, hi, dtype=np.uint16):
    lo, hi = f32(lo), f32(hi)
    p = f32([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])])
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for a, b, c, d in q for t in (a, b, c, a, c, d)], dtype)
    return p, idx


def sphere_mesh(n_lat, n_lon, radius=1.0, centre=(0.3, -0.2, 0.1), dtype=np.uint32):
    """a UV sphere of 2 n_lon (n_lat - 1) triangles"""
    pts = [(0.0, 0.0, 1.0)]
    for a in range(1, n_lat):
        t = np.pi * a / n_lat
        for b in range(n_lon):
            ph = 2 * np.pi * b / n_lon
            pts.append((np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.cos(t)))
    pts.append((0.0, 0.0, -1.0))
    p = (f32(pts) * F(radius) + f32(centre)).astype(np.float32)
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon
    idx = []
    for b in range(n_lon):
        idx += [0, ring(1, b), ring(1, b + 1)]
        idx += [len(pts) - 1, ring(n_lat - 1, b + 1), ring(n_lat - 1, b)]
    for a in range(1, n_lat - 1):
        for b in range(n_lon):
            idx += [ring(a, b), ring(a + 1, b), ring(a + 1, b + 1), ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)]
    return p, np.array(idx, dtype)


def strided(p, floats_per_vertex, fill=123.0):
    """the positions at the start of records of `floats_per_vertex` floats (a vertex stride above 12)"""
    a = np.full((len(p), floats_per_vertex), fill, np.float32)
    a[:, :3] = p
    return a


# The seed of "bottom layer": voxel 0's first ray draws z = 0.737..., then y = 0.375 and x = 1 exactly, so dir = (1, -0.25, 0.47...) and p.y is
# exactly 0 at castRay's first comparison, with an occupied cell under p: `p.y > 0` ends the march without a hit, `>=` would sample and hit.
# Built, not found by chance (two draws inside windows of 128 values each): choose v by a search over 2^24 seeds for the low halves of the
# second and third draw, derive the u state behind the second draw from the high halves, and step that multiply-with-carry half backwards
# twice (x <- x 2^16 mod m).
BOUNDARY_SEED = (1824158168, 1797839)
# The seed of "bottom layer, reciprocal", built the same way: the largest component is m = 0.9345126152038574 and y is -m / 4 exactly, so the
# true quotient y / m is -0.25 (p.y = 0: the march ends) while y * (1.0f / m), what `dir /= m` computes, is -0.24999998509883881 (p.y > 0: the
# march samples the occupied cell and hits).
RECIPROCAL_SEED = (1318498855, 481684)


def cases():
    """name -> dict(meshes=[(positions, indices)], max_res, begin=(min, max) or None for voxelize, ao=[ray_count, ...] (the first call takes
    `seed`, every further one continues the stream), seed)"""
    out = {}
    cube = box_mesh((0, 0, 0), (1, 1, 1))
    out["cube"] = dict(meshes=[cube], max_res=4, begin=None, ao=[64, 65], seed=(1234567, 7654321))
    out["slab"] = dict(meshes=[box_mesh((-1.5, 0.25, 2), (1.5, 2.25, 3), np.uint32)], max_res=9, begin=None, ao=[5], seed=(0x9E3779B9, 0x7F4A7C15))
    quad = (f32([[0, 0, 0.5], [2, 0, 0.5], [2, 1, 0.5], [0, 1, 0.5]]), np.array([0, 1, 2, 0, 2, 3], np.uint16))
    out["flat quad"] = dict(meshes=[quad], max_res=5, begin=None, ao=[1, 32], seed=(42, 4242))
    out["sphere"] = dict(meshes=[sphere_mesh(26, 40)], max_res=13, begin=None, ao=[32], seed=(0xC0FFEE, 0xBADF00D))
    # two meshes, 16- and 32-bit indices, a stride of 20 bytes, vertices no index references far outside the AABB
    p1, i1 = box_mesh((0, 0, 0), (1, 2, 1))
    p1 = np.vstack([p1, f32([[50, 50, 50], [-40, 3, 2]])])
    p2, i2 = sphere_mesh(6, 8, 0.6, (1.6, 1.0, 0.5))
    p2 = np.vstack([f32([[9, -9, 9]]), p2])
    out["two meshes"] = dict(meshes=[(strided(p1, 5), i1), (strided(p2, 7), (i2 + 1).astype(np.uint32))], max_res=8, begin=None, ao=[5], seed=(77, 99))
    # beginRaster with a box smaller than the mesh: cells fall outside the grid; a triangle larger than the grid; a zero-area triangle
    big = (f32([[-30, -20, 0.4], [40, -20, 0.6], [0, 50, 0.5], [0.5, 0.5, 0.1], [0.5, 0.5, 0.1], [0.9, 0.9, 0.9], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.8, 0.8, 0.8]]),
           np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.uint16))
    out["small box"] = dict(meshes=[big, sphere_mesh(8, 10, 1.2, (0.5, 0.5, 0.5))], max_res=6, begin=((0, 0, 0), (1, 1, 1)), ao=[5], seed=(31337, 271828))
    # the grid's bottom layer occupied (only a caller's box leaves cells there): the march's strict bounds decide voxel 0's first ray
    floor_quad = (f32([[-9, -0.2, -9], [9, -0.2, -9], [9, -0.2, 9], [-9, -0.2, 9]]), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    out["bottom layer"] = dict(meshes=[floor_quad], max_res=4, begin=((0, 0, 0), (1, 1, 1)), ao=[5], seed=BOUNDARY_SEED)
    out["bottom layer, reciprocal"] = dict(meshes=[floor_quad], max_res=4, begin=((0, 0, 0), (1, 1, 1)), ao=[5], seed=RECIPROCAL_SEED)
    return out


def lookup_points(gmn, gmx, vs):
    """points for sample / sampleAO / the bake of a grid: inside, far outside, on the max face, with a negative quotient in (-1, 0)"""
    rng = np.random.default_rng(5)
    inner = (gmn + (gmx - gmn) * f32(rng.random((24, 3)))).astype(np.float32)
    pts = [inner, f32([gmx, [gmx[0], gmn[1], gmn[2]], gmn, gmx + F(10), gmn - F(10)])]
    just_below = (gmn - vs * F(0.25)).astype(np.float32)  # quotient in (-1, 0): truncation gives cell 0
    pts.append(f32([just_below, [just_below[0], inner[0][1], inner[0][2]], [inner[1][0], inner[1][1], just_below[2]]]))
    return np.vstack(pts).astype(np.float32)


def run_case(c, **rules):
    """the whole pipeline of a case through the oracle -> dict of arrays (what the fixture records and the device must reproduce)"""
    o = Voxels(**rules)
    if c["begin"] is None:
        o.voxelize(c["meshes"], c["max_res"])
    else:
        o.beginRaster(c["begin"][0], c["begin"][1], c["max_res"])
        for p, i in c["meshes"]:
            o.raster(p, i)
    mn, mx, vs, res = o.info()
    r = dict(aabb_min=mn, aabb_max=mx, voxel_size=f32([vs]), resolution=res.astype(np.int32), voxels=o.voxels.copy())
    u, v = c["seed"]
    for k, rc in enumerate(c["ao"]):
        o.computeAO(rc, u, v)
        u, v = o.rng
        r[f"ao{k}"] = o.ao.copy()
        r[f"rng{k}"] = np.array([u, v], np.uint32)
    r["points"] = lookup_points(mn, mx, vs)
    r["sample"], r["sample_inside"] = o.sample(r["points"])
    r["sample_ao"], _ = o.sampleAO(r["points"])
    verts = np.vstack([f32(p)[:, :3] for p, _ in c["meshes"]] + [r["points"]]).astype(np.float32)
    r["bake_vertices"] = verts
    r["bake_raw_0"] = o.bakeVertexAO(verts, 0.0)  # of the AO as computeAO left it: blurAO's / 9.f (sic) lifts most of the blurred values over 1
    r["bake_raw_03"] = o.bakeVertexAO(verts, 0.3)
    o.blurAO()
    r["blurred"] = o.ao.copy()
    r["bake_0"] = o.bakeVertexAO(verts, 0.0)
    r["bake_03"] = o.bakeVertexAO(verts, 0.3)
    return r
