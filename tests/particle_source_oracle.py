"""CPU oracle of the particle VM's MESH and SPLINE instructions (ParticleSystem::run :741-798, processChunk :1189-1219,
Model::evalVertexPose model.cpp:111-129) on top of tests/particle_oracle.py and tests/ribbon_oracle.py: `run` and `process_chunk` restated
with the two instructions added, everything else as the base classes have it.

Each system carries a Source: its entity's mesh 0 (positions, skin), whether the model has bones, the pose as the matrices
computeSkinMatrices gives (the palette), and the spline's points. The deviations of DESIGN.md §4.15.2 are stated where they apply:
  a. the draw of a negative index is counter based: rand_u32 over (seed, emitter, step, particle slot, 0x80000000 + the MESH's ordinal by
     byte offset), index = float(r % n_vertices);
  b. u32(x) converts as x86-64 does (through 64 bits, low word; NaN and out of range give 0);
  c. an index >= n_vertices reads vertex 0;
  d. a bone index past the pose reads bone 0;
  e. a whole-chunk SPLINE without a spline ends the chunk's program (as the reference's `return` does): what the remaining instructions
     would have written is unspecified.
"""
import math
import struct

import numpy as np

from tests import particle_asm as A
from tests import particle_oracle as O
from tests import ribbon_oracle as R

F = np.float32
MESH_DRAW_DOMAIN = 0x80000000


def u32_x86(x):
    """u32(float) as x86-64 compiles it: cvttss2si to 64 bits, the low word (deviation b)"""
    x = float(x)
    if not math.isfinite(x) or abs(x) >= 2.0 ** 63: return 0
    return int(x) & 0xFFFFFFFF


def lerp(a, b, t):
    """core/math.cpp:190"""
    return F(F(a * F(F(1) - t)) + F(b * t))


def spline_value(points, value, sub):
    """run :785-796: clamp(u32(t), 0, size - 3) is minimum(u32, u32) (core/math.h:463, :520); rel_t = t - float(segment)"""
    n = len(points)
    with np.errstate(all="ignore"):
        t = F(F(value) * F(n - 2))
        seg = min(u32_x86(t), n - 3)
        rel = F(t - F(seg))
        p0, p1, p2 = points[seg][sub], points[seg + 1][sub], points[seg + 2][sub]
        p0 = F(F(p1 + p0) * F(0.5))
        p2 = F(F(p1 + p2) * F(0.5))
        return lerp(lerp(p0, p1, rel), lerp(p1, p2, rel), rel)


class Source:
    """What the entity of a system gives MESH and SPLINE. mesh: [n, 3] positions or None (no model instance, model not ready, no mesh);
    skin: api.SKIN records or None; has_bones: Model::getBones().size() > 0; palette: [n_bones, 4, 4] matrices as MATRIX['columns'] or None
    (no pose); spline: [n, 3] points or None (no spline component)."""

    def __init__(self, mesh=None, skin=None, has_bones=False, palette=None, spline=None):
        self.mesh = None if mesh is None else np.ascontiguousarray(mesh, F).reshape(-1, 3)
        self.skin, self.has_bones = skin, has_bones
        self.palette = None if palette is None else np.ascontiguousarray(palette, F).reshape(-1, 4, 4)
        self.spline = None if spline is None or len(spline) == 0 else np.ascontiguousarray(spline, F).reshape(-1, 3)

    def vertex(self, idx, sub):
        """mesh.vertices[idx][sub], or Model::evalVertexPose(pose, 0, idx)[sub] for a model with bones - the whole point, then the component"""
        p = self.mesh[idx]
        if not self.has_bones: return p[sub]
        w, ind = self.skin["weights"][idx], self.skin["indices"][idx]
        ms = []
        for k in range(4):
            b = int(ind[k]) & 0xFFFF
            ms.append(self.palette[b if b < len(self.palette) else 0])  # deviation d
        with np.errstate(all="ignore"):
            m = ((ms[0] * w[0] + ms[1] * w[1]) + ms[2] * w[2]) + ms[3] * w[3]  # element by element, fp32 (math.cpp:1022-1071)
            c = m  # [column][row]
            out = [F(F(F(c[0][r] * p[0]) + F(c[1][r] * p[1])) + F(c[2][r] * p[2])) + c[3][r] for r in range(3)]  # transformPoint, math.cpp:1231
        return F(out[sub])


NO_SOURCE = Source()


class SourceVM:
    """`run` and `process_chunk` with MESH and SPLINE; mixed in front of a World."""

    def source_of(self, sy):
        return getattr(sy, "source", NO_SOURCE)

    def prescan_meshes(self, em):
        """MESH ordinals by byte offset, numbered on their own: RAND's ordinals (prescan_rands) do not move"""
        code, ip, n, at_list = em.code, 0, len(em.code), []
        while ip < n:
            op = A.OPS[code[ip]]
            at = ip
            ip += 1
            if op in A.ARITY: ip += 8 * (1 + A.ARITY[op])
            elif op == "RAND": ip += 16
            elif op == "GRADIENT": ip += 16 + 4 + 8 * struct.unpack_from("<I", code, ip + 16)[0]
            elif op == "CMP": ip += 10
            elif op == "CMP_ELSE": ip += 12
            elif op == "EMIT": ip += 4
            elif op in ("MESH", "SPLINE"):
                if op == "MESH": at_list.append(at)
                ip += 17
        em.mesh_at = {a: k for k, a in enumerate(sorted(at_list))}

    # ---- ParticleSystem::run -------------------------------------------------------------------------------------------------------
    def run(self, sy, em, ip, pidx, regs, ridx, out, emitting=False, total_time=F(0), emit_index=F(0), nested=False):
        code = em.code
        box = [out]
        src = self.source_of(sy)

        def get(s):
            t, i, b = s
            if t == A.LITERAL: return np.uint32(b).view(F)
            if t == A.SYSTEM_VALUE:
                if emitting and i == A.TOTAL_TIME: return total_time
                if i == A.EMIT_INDEX: return emit_index
                return sy.sysv[i]
            if t == A.OUTPUT: return box[0][i]
            if t == A.REGISTER: return regs[i, ridx]
            if t == A.CHANNEL: return em.ch[i, pidx]
            if t == A.GLOBAL: return sy.globals[i]
            raise AssertionError("bad stream")

        def put(s, v):
            t, i, _ = s
            v = F(v)
            if t == A.OUTPUT: box[0][i] = v
            elif t == A.REGISTER: regs[i, ridx] = v
            elif t == A.CHANNEL: em.ch[i, pidx] = v
            else: raise AssertionError("bad destination")

        end_counter, killed, skip_stack = 1, False, []
        with np.errstate(all="ignore"):
            while True:
                at = ip
                op = A.OPS[code[ip]]
                ip += 1
                if op == "END":
                    if skip_stack:
                        ip += skip_stack.pop()
                        continue
                    end_counter -= 1
                    if end_counter > 0: continue
                    return ip if nested else killed
                if op == "EMIT":
                    target = struct.unpack_from("<I", code, ip)[0]
                    outs = np.zeros(16, F)
                    ip = self.run(sy, em, ip + 4, pidx, regs, ridx, outs, emitting, total_time, emit_index, nested=True)
                    em.emit_stream.append((target, outs[:sy.emitters[target].p.emit_inputs].copy()))
                    continue
                if op == "KILL":
                    killed = True
                    continue
                if op == "MESH":  # :741-774; every `return` is the reference's early return with the verdict so far
                    assert not nested, "MESH inside an EMIT block is refused"
                    dst, ip = self._ds(code, ip)
                    index, ip = self._ds(code, ip)
                    sub = code[ip]
                    ip += 1
                    if src.mesh is None: return killed
                    n = len(src.mesh)
                    if get(index) < 0:  # deviation a
                        put(index, F(O.rand_u32(self.seed, em.gid, self.step_no, pidx, MESH_DRAW_DOMAIN + em.mesh_at[at]) % n))
                    if src.has_bones and src.palette is None: return killed
                    idx = u32_x86(F(get(index) + F(0.5)))
                    if idx >= n: idx = 0  # deviation c
                    put(dst, src.vertex(idx, sub))
                    continue
                if op == "SPLINE":  # :775-798
                    assert not nested, "SPLINE inside an EMIT block is refused"
                    dst, ip = self._ds(code, ip)
                    s, ip = self._ds(code, ip)
                    sub = code[ip]
                    ip += 1
                    if src.spline is None: return killed
                    put(dst, spline_value(src.spline, get(s), sub))
                    continue
                if op == "RAND":
                    dst, ip = self._ds(code, ip)
                    lo, hi = struct.unpack_from("<ff", code, ip)
                    ip += 8
                    put(dst, O.rand_float(lo, hi, O.rand_u32(self.seed, em.gid, self.step_no, pidx, em.rand_at[at])))
                    continue
                if op == "CMP":
                    c, ip = self._ds(code, ip)
                    ts = struct.unpack_from("<H", code, ip)[0]
                    ip += 2
                    if get(c) != 0: end_counter += 1
                    else: ip += ts
                    continue
                if op == "CMP_ELSE":
                    c, ip = self._ds(code, ip)
                    ts, fs = struct.unpack_from("<HH", code, ip)
                    ip += 4
                    if get(c) != 0: skip_stack.append(fs)
                    else:
                        ip += ts
                        end_counter += 1
                    continue
                dst, ip = self._ds(code, ip)
                srcs = []
                for _ in range(A.ARITY[op]):
                    s, ip = self._ds(code, ip)
                    srcs.append(get(s))
                a = srcs[0]
                b = srcs[1] if len(srcs) > 1 else None
                if op == "MUL": v = a * b
                elif op == "ADD": v = a + b
                elif op == "SUB": v = a - b
                elif op == "DIV": v = np.divide(a, b)
                elif op == "MOD": v = np.fmod(a, b)
                elif op == "MULTIPLY_ADD": v = F(a * b) + srcs[2]
                elif op == "MIX": v = F(a * F(F(1) - srcs[2])) + F(b * srcs[2])
                elif op == "AND": v = F(1) if (a != 0 and b != 0) else F(0)
                elif op == "OR": v = F(1) if (a != 0 or b != 0) else F(0)
                elif op == "NOT": v = O.ALL_ONES if a == 0 else F(0)
                elif op == "MOV": v = a
                elif op == "SIN": v = O.sinf(a)
                elif op == "COS": v = O.cosf(a)
                elif op == "SQRT": v = np.sqrt(a)
                elif op == "NOISE": v = O.gnoise(a)
                elif op == "MAX": v = a if a > b else b
                elif op == "MIN": v = a if a < b else b
                elif op == "LT": v = F(1) if a < b else F(0)
                elif op == "GT": v = F(1) if a > b else F(0)
                else: raise AssertionError(op)
                put(dst, v)

    # ---- processChunk --------------------------------------------------------------------------------------------------------------
    def process_chunk(self, sy, em, frm, to, offset, out, kill_counter):
        """The base class's processChunk with the whole-chunk SPLINE case (:1189-1219) added."""
        code, ip = em.code, offset
        n4 = (to - frm + 3) & ~3
        sl = slice(frm, frm + n4)
        regs = np.zeros((16, O.CHUNK), F)
        nout = em.p.outputs
        rows = np.arange(frm, frm + n4)
        src = self.source_of(sy)
        bits = O.bits

        def arg(s):
            t, i, b = s
            if t == A.CHANNEL: return em.ch[i, sl].copy()
            if t == A.REGISTER: return regs[i, :n4].copy()
            if t == A.LITERAL: return np.full(n4, np.uint32(b).view(F), F)
            if t == A.SYSTEM_VALUE: return np.full(n4, F(0) if i == A.EMIT_INDEX else sy.sysv[i], F)
            if t == A.GLOBAL: return np.full(n4, sy.globals[i], F)
            raise AssertionError("bad stream")

        def put(s, v):
            t, i, _ = s
            v = np.asarray(v, F)
            if t == A.OUTPUT: out[rows * nout + i] = v
            elif t == A.CHANNEL: em.ch[i, sl] = v
            elif t == A.REGISTER: regs[i, :n4] = v
            else: raise AssertionError("bad destination")

        def mask(c):
            return np.where(c, np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32).view(F)

        with np.errstate(all="ignore"):
            while True:
                at = ip
                op = A.OPS[code[ip]]
                ip += 1
                if op == "END": return
                if op == "SPLINE":  # :1189-1219
                    dst, ip = self._ds(code, ip)
                    s, ip = self._ds(code, ip)
                    sub = code[ip]
                    ip += 1
                    assert dst[0] == A.OUTPUT
                    if src.spline is None: return  # deviation e: the rest of this chunk's program does not run
                    put(dst, [spline_value(src.spline, x, sub) for x in arg(s)])
                    continue
                if op in ("CMP", "CMP_ELSE"):
                    c, ip = self._ds(code, ip)
                    if op == "CMP":
                        ts, fs = struct.unpack_from("<H", code, ip)[0], 0
                        ip += 2
                    else:
                        ts, fs = struct.unpack_from("<HH", code, ip)
                        ip += 4
                    t_ip, f_ip = ip, ip + ts
                    ip += ts + fs
                    cond = bits(arg(c)) >> 31
                    kill_count, last = 0, to - 1
                    for k in range(n4):
                        pi = frm + k
                        is_true = bool(cond[k]) and pi < to
                        if not is_true and op == "CMP": continue
                        o = out[pi * nout:(pi + 1) * nout] if out is not None else None
                        if self.run(sy, em, t_ip if is_true else f_ip, pi, regs, k, o):
                            if last >= frm: em.ch[:, pi] = em.ch[:, last]
                            last -= 1
                            kill_count += 1
                    if kill_count > 0: kill_counter[frm // O.CHUNK] = kill_count
                    continue
                if op == "RAND":
                    dst, ip = self._ds(code, ip)
                    lo, hi = struct.unpack_from("<ff", code, ip)
                    ip += 8
                    put(dst, [O.rand_float(lo, hi, O.rand_u32(self.seed, em.gid, self.step_no, frm + k, em.rand_at[at])) for k in range(n4)])
                    continue
                if op == "GRADIENT":
                    dst, ip = self._ds(code, ip)
                    s, ip = self._ds(code, ip)
                    cnt = struct.unpack_from("<I", code, ip)[0]
                    keys = np.array(struct.unpack_from(f"<{cnt}f", code, ip + 4), F)
                    vals = np.array(struct.unpack_from(f"<{cnt}f", code, ip + 4 + 4 * cnt), F)
                    ip += 4 + 8 * cnt
                    ms = np.zeros(cnt, F)
                    ms[1:] = (vals[1:] - vals[:-1]) / (keys[1:] - keys[:-1])
                    res = np.zeros(n4, F)
                    for k, x in enumerate(arg(s)):
                        m = x if x > keys[0] else keys[0]
                        v = m if m < keys[cnt - 1] else keys[cnt - 1]
                        j = 1
                        while j + 1 < cnt and v > keys[j]: j += 1
                        res[k] = vals[j] - F(F(keys[j] - v) * ms[j])
                    put(dst, res)
                    continue
                dst, ip = self._ds(code, ip)
                srcs = []
                for _ in range(A.ARITY[op]):
                    s, ip = self._ds(code, ip)
                    srcs.append(arg(s))
                a = srcs[0]
                b = srcs[1] if len(srcs) > 1 else None
                if op == "MUL": v = a * b
                elif op == "ADD": v = a + b
                elif op == "SUB": v = a - b
                elif op == "DIV": v = a / b
                elif op == "MOD": v = np.fmod(a, b)
                elif op == "MULTIPLY_ADD": v = (a * b) + srcs[2]
                elif op == "MIX": v = a + (b - a) * srcs[2]
                elif op == "BLEND": v = np.where(bits(srcs[2]) >> 31 != 0, b, a)
                elif op == "AND": v = (bits(a) & bits(b)).view(F)
                elif op == "OR": v = (bits(a) | bits(b)).view(F)
                elif op == "MOV": v = a
                elif op == "SIN": v = O.vsinf(a)
                elif op == "COS": v = O.vcosf(a)
                elif op == "SQRT": v = np.sqrt(a)
                elif op == "NOISE": v = np.array([O.gnoise(x) for x in a], F)
                elif op == "MAX": v = np.where(a > b, a, b)
                elif op == "MIN": v = np.where(a < b, a, b)
                elif op == "LT": v = mask(a < b)
                elif op == "GT": v = mask(a > b)
                else: raise AssertionError(op)
                put(dst, v)


class World(SourceVM, O.World):
    pass


class RibbonWorld(SourceVM, R.World):
    pass


def make_world(programs_by_system, capacities, sources=None, options=None, seed=0, n_globals=0, positions=None):
    """As the base make_world functions; sources: one Source per system (None: none declared). With `options` the world is a RibbonWorld."""
    systems = []
    for si, progs in enumerate(programs_by_system):
        cap = lambda ei: capacities if isinstance(capacities, int) else capacities[si][ei]
        if options is not None: ems = [R.Emitter(p, cap(ei), options[si][ei]) for ei, p in enumerate(progs)]
        else: ems = [O.Emitter(p, cap(ei)) for ei, p in enumerate(progs)]
        sy = O.System(ems, n_globals, tuple(positions[si]) if positions is not None else (0.0, 0.0, 0.0))
        sy.source = sources[si] if sources is not None and sources[si] is not None else NO_SOURCE
        systems.append(sy)
    w = (RibbonWorld if options is not None else World)(systems, seed)
    for s in systems:
        for e in s.emitters:
            w.prescan_rands(e)
            w.prescan_meshes(e)
    return w
