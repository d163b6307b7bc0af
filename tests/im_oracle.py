"""CPU oracle of the instanced-model path: a plain restatement, in numpy, of

  1. RenderModuleImpl::initInstancedModelGPUData (renderer/render_module.cpp:1285-1365): grid AABB (AABB::addPoint = minCoords /
     maxCoords, a NaN coordinate never wins), 4 x 4 XZ cells, shrink(-0.01f), each instance to the FIRST cell whose AABB::contains
     (core/geometry.cpp:540-548) accepts it, stable scatter. Instances no cell accepts follow the placed ones in input order (the
     reference leaves the default-initialised records of Array::resize in those slots; they belong to no cell and are never drawn).
  2. the cell pass of PipelineImpl::encodeInstancedModels (renderer/pipeline.cpp:2507-2545): visible = ShiftedFrustum::getRelative(origin)
     .intersectAABBWithOffset(cell, radius) (geometry.cpp:121-149, :58-75), near = length(origin - cam + center) - cell_radius < draw
     distance in fp64.
  3. data/shaders/instancing.hlsl: getLOD, the cross-fade (visible cells of non-shadow views), the snap (near-but-invisible cells of
     non-shadow views), cull(), the bins floor(lod) / floor(lod) + 1 with w = frac / frac - 1.
  4. PASS2: one indirect record per mesh.

Every fp32 operation is one numpy float32 operation (no fused multiply-add), in the order written in the reference; the shader's dot
products are taken left to right (HLSL's order is the reference GPU compiler's choice: a transcription). Layout deviations of the port,
restated here as the port defines them: model m's records start behind every record of models 0..m-1, bin b behind bins 0..b-1 of the
model, records inside a bin in ascending instance order; every model owns mesh_count indirect slots."""
import numpy as np

F = np.float32
FLT_MAX = np.float32(np.finfo(np.float32).max)
PLANE_POINT = [0, 4, 1, 0, 0, 2]  # getRelative re-anchors NEAR, FAR, LEFT, RIGHT, TOP, BOTTOM on these corner points

IM_INSTANCE = np.dtype([("rot", "<f4", 3), ("lod", "<f4"), ("pos", "<f4", 3), ("scale", "<f4")])


def grid_build(inst):
    """-> (sorted instances, grid dict: min, max, cmin[16,3], cmax[16,3], from[16], count[16], placed, unplaced)"""
    inst = np.ascontiguousarray(inst, IM_INSTANCE)
    pos = inst["pos"].astype(F)
    mn = np.full(3, FLT_MAX, F)
    mx = np.full(3, -FLT_MAX, F)
    for k in range(3):
        col = pos[:, k][~np.isnan(pos[:, k])]
        if len(col):
            lo, hi = col.min(), col.max()
            mn[k] = lo if lo < mn[k] else mn[k]
            mx[k] = hi if hi > mx[k] else mx[k]
    with np.errstate(all="ignore"):
        csx = (mx[0] - mn[0]) * F(0.25)
        csz = (mx[2] - mn[2]) * F(0.25)
        cmin = np.zeros((16, 3), F)
        cmax = np.zeros((16, 3), F)
        for j in range(4):
            for i in range(4):
                c = i + 4 * j
                cmin[c] = [mn[0] + csx * F(i), mn[1], mn[2] + csz * F(j)]
                cmax[c] = [cmin[c, 0] + csx, mx[1], cmin[c, 2] + csz]
        cmin = cmin + F(-0.01)
        cmax = cmax - F(-0.01)
    cell = np.full(len(inst), 16, np.int64)
    for c in range(16):
        inside = ~((cmin[c, 0] > pos[:, 0]) | (cmin[c, 1] > pos[:, 1]) | (cmin[c, 2] > pos[:, 2]) | (pos[:, 0] > cmax[c, 0]) | (pos[:, 1] > cmax[c, 1]) |
                   (pos[:, 2] > cmax[c, 2]))
        cell[(cell == 16) & inside] = c
    order = np.argsort(cell, kind="stable")
    count = np.bincount(cell, minlength=17)
    frm = np.concatenate([[0], np.cumsum(count)])[:17]
    g = {"min": mn, "max": mx, "cmin": cmin, "cmax": cmax, "from": frm[:16].astype(np.uint32), "count": count[:16].astype(np.uint32),
         "placed": int(count[:16].sum()), "unplaced": int(count[16])}
    return inst[order].copy(), g


def cell_verdicts(g, origin, radius, draw_distance, cam, frustum):
    """0 skipped, 1 near but not visible, 2 visible (pipeline.cpp:2507-2545)"""
    fr = frustum.reshape(-1)[0]
    origin = np.asarray(origin, np.float64)
    offset = (fr["origin"].astype(np.float64) - origin).astype(F)
    out = np.zeros(16, np.int64)
    with np.errstate(all="ignore"):
        for c in range(16):
            if g["count"][c] == 0:
                continue
            mn, mx = g["cmin"][c], g["cmax"][c]
            visible = True
            for k in range(6):
                n = np.array([fr["xs"][k], fr["ys"][k], fr["zs"][k]], F)
                q = fr["points"][PLANE_POINT[k]].astype(F) + offset
                d = -((q[0] * n[0] + q[1] * n[1]) + q[2] * n[2])
                b = np.where(n > 0, mx, mn)
                dp = (n[0] * b[0] + n[1] * b[1]) + n[2] * b[2]
                if dp < -d - F(radius):
                    visible = False
            center = (mx + mn) * F(0.5)
            half = (mx - mn) * F(0.5)
            cell_radius = np.sqrt((half[0] * half[0] + half[1] * half[1]) + half[2] * half[2])
            rel = (origin - np.asarray(cam, np.float64)) + center.astype(np.float64)
            length = np.sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2])
            if length - np.float64(cell_radius) < np.float64(F(draw_distance)):
                out[c] = 2 if visible else 1
    return out


def draw_distance(lod_dist, lod_idx):
    dist = F(0)
    for k in range(4):
        if lod_idx[k][1] != -1:
            dist = F(lod_dist[k])
    with np.errstate(invalid="ignore"):
        return np.sqrt(dist)  # a distance below 0 with to != -1: NaN, as sqrtf gives


class Oracle:
    def __init__(self):
        self.models = []

    def set_model(self, m, lod_distances, lod_indices, radius, indices_count):
        rec = {"lod_dist": np.asarray(lod_distances, F).reshape(4), "lod_idx": np.asarray(lod_indices, np.int64).reshape(5, 2), "radius": F(radius),
               "indices": np.asarray(indices_count, np.uint32), "inst": np.zeros(0, IM_INSTANCE), "grid": grid_build(np.zeros(0, IM_INSTANCE))[1],
               "origin": np.zeros(3)}
        if m == len(self.models):
            self.models.append(rec)
        else:
            rec["inst"], rec["grid"], rec["origin"] = self.models[m]["inst"], self.models[m]["grid"], self.models[m]["origin"]
            self.models[m] = rec

    def set_instances(self, m, inst):
        self.models[m]["inst"], self.models[m]["grid"] = grid_build(inst)

    def set_origins(self, pos):
        for m, p in enumerate(np.asarray(pos, np.float64).reshape(-1, 3)):
            self.models[m]["origin"] = p.copy()

    def run(self, view, frustum):
        """-> (counts: list of dicts, records IM_INSTANCE[], indirect uint32[k, 5]); LODs updated in place"""
        view = view.reshape(-1)[0]
        fr = frustum.reshape(-1)[0]
        cam = view["camera_pos"].astype(np.float64)
        shadow = bool(view["is_shadow"])
        planes = np.stack([fr["xs"][:6], fr["ys"][:6], fr["zs"][:6], fr["ds"][:6]], 1).astype(F)
        counts, recs, indirect = [], [], []
        base = 0
        for md in self.models:
            inst, g = md["inst"], md["grid"]
            lod_idx = [int(md["lod_idx"][0][1])]
            for k in range(1, 4):
                lod_idx.append(max(lod_idx[-1], int(md["lod_idx"][k][1])))
            verdict = cell_verdicts(g, md["origin"], md["radius"], draw_distance(md["lod_dist"], md["lod_idx"]), cam, frustum)
            placed = g["placed"]
            cell_of = np.repeat(np.arange(16), g["count"].astype(np.int64))
            v = verdict[cell_of] if placed else np.zeros(0, np.int64)
            co = (md["origin"] - cam).astype(F)
            with np.errstate(all="ignore"):
                ld = md["lod_dist"] * F(view["lod_multiplier"])
                ld = np.where(ld < 0, FLT_MAX, ld).astype(F)
                ps = inst["pos"][:placed].astype(F)
                scale = inst["scale"][:placed].astype(F)
                px, py, pz = ps[:, 0] + co[0], ps[:, 1] + co[1], ps[:, 2] + co[2]
                lod = inst["lod"][:placed].copy()
                if not shadow:
                    d = (px * px + py * py) + pz * pz
                    dst = np.where(d > ld[3], F(4), np.where(d > ld[2], F(3), np.where(d > ld[1], F(2), np.where(d > ld[0], F(1), F(0))))).astype(F)
                    td = F(view["time_delta"]) * F(2)
                    dd = dst - lod
                    sgn = ((dd > 0).astype(np.int32) - (dd < 0).astype(np.int32)).astype(F)
                    fade = np.where(np.abs(dd) < td, dst, lod + td * sgn).astype(F)
                    lod = np.where(v == 2, fade, np.where(v == 1, dst, lod)).astype(F)
                    inst["lod"][:placed] = lod
                passes = np.ones(placed, bool)
                sr = md["radius"] * scale
                for k in range(6):
                    dp = ((planes[k, 0] * px + planes[k, 1] * py) + planes[k, 2] * pz) + planes[k, 3]
                    passes &= ~(dp < -sr)
                emit = (v == 2) & (lod <= F(3)) & passes
                b0 = np.where(lod > 0, np.trunc(np.where(emit, lod, F(0))), 0).astype(np.int64)
                t = (lod - np.floor(lod)).astype(F)
                two = emit & (t > F(0.01))
                tot, offs = [], []
                model_recs = []
                for b in range(4):
                    first = emit & (b0 == b)
                    second = two & (b0 + 1 == b)
                    sel = np.flatnonzero(first | second)
                    r = np.zeros(len(sel), IM_INSTANCE)
                    r["rot"] = inst["rot"][sel]
                    r["lod"] = np.where(first[sel], t[sel], t[sel] - F(1))
                    r["pos"] = np.stack([px[sel], py[sel], pz[sel]], 1)
                    r["scale"] = scale[sel] + F(0)
                    tot.append(len(sel))
                    model_recs.append(r)
            off = [base]
            for b in range(3):
                off.append(off[-1] + tot[b])
            for i in range(len(md["indices"])):
                rec = [int(md["indices"][i]), 0, 0, 0, 0]
                if i <= lod_idx[3]:
                    b = 0 if i <= lod_idx[0] else 1 if i <= lod_idx[1] else 2 if i <= lod_idx[2] else 3
                    rec[1], rec[4] = tot[b], off[b]
                indirect.append(rec)
            counts.append({"bin_count": tot, "bin_offset": off, "unplaced": g["unplaced"], "instances": len(inst), "verdict": verdict})
            recs.extend(model_recs)
            base += sum(tot)
        records = np.concatenate(recs) if recs else np.zeros(0, IM_INSTANCE)
        return counts, records, np.asarray(indirect, np.uint32).reshape(-1, 5)


def unplaced_field(n=20000, seed=5):
    """x spans [615636.3125, 619811.4375] (ulp 1/16: the cells' 0.01 margins round away) and the last cell's max, min.x + 3 cs + cs in fp32,
    rounds below the grid's max.x: the instances at max.x lie in no cell."""
    rng = np.random.default_rng(seed)
    inst = np.zeros(n, IM_INSTANCE)
    inst["pos"][:, 0] = rng.uniform(615636.3125, 619811.4375, n).astype(np.float32)
    inst["pos"][:, 2] = rng.uniform(-500, 500, n).astype(np.float32)
    inst["pos"][0, 0], inst["pos"][1::97, 0] = np.float32(615636.3125), np.float32(619811.4375)
    inst["scale"] = 1
    inst["lod"] = rng.uniform(0, 4, n).astype(np.float32)
    return inst
