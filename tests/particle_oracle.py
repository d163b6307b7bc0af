"""CPU oracle of the particle systems: a plain-Python / numpy restatement of ParticleSystem::update, emit, processChunk, run, the
cross-chunk compaction and Emitter::fillInstanceData (renderer/particle_system.cpp), interpreting the byte stream itself.

The deviations of DESIGN.md §4.15 are stated where they apply:
  1. whole-chunk instructions take the intrinsic form of core/simd.h (sign-bit masks, bitwise AND / OR, _mm_min_ps / _mm_max_ps);
  2. kills are the literal sequential loop;
  3. registers inside conditional blocks are indexed chunk-locally;
  5. RAND is the counter-based draw through RandomGenerator::randFloat's formula;
  6. gnoise converts u32(floor(p)) as x86-64 does;
  8. capacity is reserved: an emission past it is counted and not written.
EMIT_INDEX outside the emit program reads 0 and the register pages start as zeros (the reference leaves both to chance).
"""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

from tests import particle_asm as A

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
for _n in ("sinf", "cosf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]
CHUNK = 1024
ALL_ONES = np.uint32(0xFFFFFFFF).view(F)


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def sinf(x): return F(_libm.sinf(float(x)))
def cosf(x): return F(_libm.cosf(float(x)))
def vsinf(a): return np.array([_libm.sinf(float(x)) for x in a], F)
def vcosf(a): return np.array([_libm.cosf(float(x)) for x in a], F)


def mix32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def rand_u32(seed, emitter, step, particle, ordinal):
    r = mix32(seed ^ 0x9E3779B9)
    for k in (emitter, step, particle, ordinal):
        r = mix32(r ^ k)
    return r


def rand_float(lo, hi, r):
    """RandomGenerator::randFloat(from, to) fed the u32 `r` (core/math.cpp:1372)"""
    lo, hi = F(lo), F(hi)
    return F(lo + F(float(F(hi - lo)) * (r * 2.328306435996595e-10)))


def hash_u32(n):
    n &= 0xFFFFFFFF
    n = ((n << 13) & 0xFFFFFFFF) ^ n
    n = (n * ((n * n * 15731 + 789221) & 0xFFFFFFFF) + 1376312589) & 0xFFFFFFFF
    return F(F(n & 0x0FFFFFFF) / F(0x0FFFFFFF))


def gnoise(p):
    p = F(p)
    fl = math.floor(float(p)) if math.isfinite(float(p)) else None
    i = (fl & 0xFFFFFFFF) if fl is not None and abs(fl) < 2 ** 63 else 0  # cvttss2si r64, low word
    with np.errstate(all="ignore"):
        f = F(p - F(i))
        u = F(F(F(f * f) * f) * F(F(f * F(F(f * F(6)) - F(15))) + F(10)))
        v0, v1 = hash_u32(i), hash_u32(i + 1)
        return F(F(F(F(v0 * F(F(1) - u)) + F(v1 * u)) - F(0.5)) * F(4.8))


class Emitter:
    def __init__(self, prog: A.Program, capacity: int):
        self.p = prog
        self.code = prog.bytes
        self.capacity = (capacity + 3) & ~3
        self.ch = np.zeros((prog.channels, self.capacity), F)
        self.count = self.emit_index = self.overflow = self.killed = 0
        self.emit_timer = F(0)
        # ordinals of the RAND instructions: their order in the stream (update | emit | output)
        self.rand_at = {}
        self.emit_stream = []  # (target emitter, emit outputs) in the order the update appended them


class System:
    def __init__(self, emitters, n_globals=0, pos=(0.0, 0.0, 0.0)):
        self.emitters = emitters
        self.globals = np.zeros(n_globals, F)
        self.pos = pos
        self.total_time = F(0)
        self.sysv = np.zeros(7, F)


class World:
    def __init__(self, systems, seed=0):
        self.systems = systems
        self.seed = seed
        self.step_no = 0
        g = 0
        for s in systems:
            for e in s.emitters:
                e.gid = g
                g += 1

    # ---- the byte stream ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _ds(code, ip):
        t, i, v = struct.unpack_from("<BBxxf", code, ip)
        return (t, i, struct.unpack_from("<I", code, ip + 4)[0]), ip + 8

    def prescan_rands(self, em):
        """RAND ordinals must not depend on which instruction ran first: walk the whole stream once."""
        code, ip, n = em.code, 0, len(em.code)
        while ip < n:
            op = A.OPS[code[ip]]
            at = ip
            ip += 1
            if op in A.ARITY: ip += 8 * (1 + A.ARITY[op])
            elif op == "RAND":
                em.rand_at[at] = None
                ip += 16
            elif op == "GRADIENT": ip += 16 + 4 + 8 * struct.unpack_from("<I", code, ip + 16)[0]
            elif op == "CMP": ip += 10
            elif op == "CMP_ELSE": ip += 12
            elif op == "EMIT": ip += 4
            elif op in ("MESH", "SPLINE"): ip += 17
        for k, a in enumerate(sorted(em.rand_at)):
            em.rand_at[a] = k

    # ---- ParticleSystem::run -------------------------------------------------------------------------------------------------------
    def run(self, sy, em, ip, pidx, regs, ridx, out, emitting=False, total_time=F(0), emit_index=F(0), nested=False):
        """True when the particle was killed (nested, the EMIT block's own run: the position behind its END)"""
        code = em.code
        box = [out]  # where OUT operands go: the particle's output row, or an EMIT block's outputs

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
                if op == "EMIT":  # :958-983: the block runs with its outputs redirected, then the record is appended
                    target = struct.unpack_from("<I", code, ip)[0]
                    outs = np.zeros(16, F)
                    ip = self.run(sy, em, ip + 4, pidx, regs, ridx, outs, emitting, total_time, emit_index, nested=True)
                    em.emit_stream.append((target, outs[:sy.emitters[target].p.emit_inputs].copy()))
                    continue
                if op == "KILL":
                    killed = True
                    continue
                if op == "RAND":
                    dst, ip = self._ds(code, ip)
                    lo, hi = struct.unpack_from("<ff", code, ip)
                    ip += 8
                    put(dst, rand_float(lo, hi, rand_u32(self.seed, em.gid, self.step_no, pidx, em.rand_at[at])))
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
                src = []
                for _ in range(A.ARITY[op]):
                    s, ip = self._ds(code, ip)
                    src.append(get(s))
                a = src[0]
                b = src[1] if len(src) > 1 else None
                if op == "MUL": v = a * b
                elif op == "ADD": v = a + b
                elif op == "SUB": v = a - b
                elif op == "DIV": v = np.divide(a, b)
                elif op == "MOD": v = np.fmod(a, b)
                elif op == "MULTIPLY_ADD": v = F(a * b) + src[2]
                elif op == "MIX": v = F(a * F(F(1) - src[2])) + F(b * src[2])
                elif op == "AND": v = F(1) if (a != 0 and b != 0) else F(0)
                elif op == "OR": v = F(1) if (a != 0 or b != 0) else F(0)
                elif op == "NOT": v = ALL_ONES if a == 0 else F(0)
                elif op == "MOV": v = a
                elif op == "SIN": v = sinf(a)
                elif op == "COS": v = cosf(a)
                elif op == "SQRT": v = np.sqrt(a)
                elif op == "NOISE": v = gnoise(a)
                elif op == "MAX": v = a if a > b else b
                elif op == "MIN": v = a if a < b else b
                elif op == "LT": v = F(1) if a < b else F(0)
                elif op == "GT": v = F(1) if a > b else F(0)
                else: raise AssertionError(op)
                put(dst, v)

    # ---- ParticleSystem::emit ------------------------------------------------------------------------------------------------------
    def emit(self, sy, em, count, time_step, c1, emit_data=()):
        regs = np.zeros((16, 1), F)
        t = F(c1)
        for _ in range(count):
            if em.count < em.capacity:
                regs[:] = 0
                regs[:len(emit_data), 0] = emit_data
                self.run(sy, em, em.p.emit_offset, em.count, regs, 0, None, True, t, F(em.emit_index))
                em.count += 1
            else:
                em.overflow = 1
            em.emit_index += 1
            t = F(t + F(time_step))

    # ---- processChunk --------------------------------------------------------------------------------------------------------------
    def process_chunk(self, sy, em, frm, to, offset, out, kill_counter):
        code, ip = em.code, offset
        n4 = (to - frm + 3) & ~3
        sl = slice(frm, frm + n4)
        regs = np.zeros((16, CHUNK), F)
        nout = em.p.outputs
        rows = np.arange(frm, frm + n4)

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
                    cond = bits(arg(c)) >> 31  # f4MoveMask of the intrinsic form: the sign bit
                    kill_count, last = 0, to - 1
                    for k in range(n4):
                        pi = frm + k
                        is_true = bool(cond[k]) and pi < to
                        if not is_true and op == "CMP": continue
                        o = out[pi * nout:(pi + 1) * nout] if out is not None else None
                        if self.run(sy, em, t_ip if is_true else f_ip, pi, regs, k, o):  # deviation 3: register index k, not pi
                            if last >= frm: em.ch[:, pi] = em.ch[:, last]  # (below the chunk: outside what is defined, nothing moves)
                            last -= 1
                            kill_count += 1
                    if kill_count > 0: kill_counter[frm // CHUNK] = kill_count
                    continue
                if op == "RAND":
                    dst, ip = self._ds(code, ip)
                    lo, hi = struct.unpack_from("<ff", code, ip)
                    ip += 8
                    put(dst, [rand_float(lo, hi, rand_u32(self.seed, em.gid, self.step_no, frm + k, em.rand_at[at])) for k in range(n4)])
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
                src = []
                for _ in range(A.ARITY[op]):
                    s, ip = self._ds(code, ip)
                    src.append(arg(s))
                a = src[0]
                b = src[1] if len(src) > 1 else None
                if op == "MUL": v = a * b
                elif op == "ADD": v = a + b
                elif op == "SUB": v = a - b
                elif op == "DIV": v = a / b
                elif op == "MOD": v = np.fmod(a, b)
                elif op == "MULTIPLY_ADD": v = (a * b) + src[2]
                elif op == "MIX": v = a + (b - a) * src[2]
                elif op == "BLEND": v = np.where(bits(src[2]) >> 31 != 0, b, a)
                elif op == "AND": v = (bits(a) & bits(b)).view(F)
                elif op == "OR": v = (bits(a) | bits(b)).view(F)
                elif op == "MOV": v = a
                elif op == "SIN": v = vsinf(a)
                elif op == "COS": v = vcosf(a)
                elif op == "SQRT": v = np.sqrt(a)
                elif op == "NOISE": v = np.array([gnoise(x) for x in a], F)
                elif op == "MAX": v = np.where(a > b, a, b)  # _mm_max_ps
                elif op == "MIN": v = np.where(a < b, a, b)
                elif op == "LT": v = mask(a < b)
                elif op == "GT": v = mask(a > b)
                else: raise AssertionError(op)
                put(dst, v)

    # ---- ParticleSystem::update(dt, emitter_idx) -------------------------------------------------------------------------------------
    def update_emitter(self, sy, em, dt):
        p = em.p
        if p.emit_per_second > 0:
            em.emit_timer = F(em.emit_timer + F(dt))
            if em.emit_timer > 0:
                d = F(F(1) / F(p.emit_per_second))
                count = int(math.floor(float(F(em.emit_timer / d))))
                self.emit(sy, em, count, d, sy.total_time)
                em.emit_timer = F(em.emit_timer - F(d * F(count)))
        em.killed = 0
        if em.count == 0: return
        chunks = (em.count + CHUNK - 1) // CHUNK
        kc = [0] * chunks
        for frm in range(0, em.count, CHUNK):
            self.process_chunk(sy, em, frm, min(frm + CHUNK, em.count), 0, None, kc)
        head, tail, total = 0, chunks - 1, sum(kc)
        while head != tail:
            if kc[head] == 0:
                head += 1
                continue
            tail_start = CHUNK * tail
            tail_count = min(CHUNK, em.count - tail_start) - kc[tail]
            dst = head * CHUNK + CHUNK - kc[head]
            if tail_count <= kc[head]:
                em.ch[:, dst:dst + tail_count] = em.ch[:, tail_start:tail_start + tail_count]
                tail -= 1
                kc[head] -= tail_count
            else:
                src = tail_start + tail_count - kc[head]
                em.ch[:, dst:dst + kc[head]] = em.ch[:, src:src + kc[head]]
                kc[tail] += kc[head]
                head += 1
        em.killed = total
        em.count -= total
        stream, em.emit_stream = em.emit_stream, []
        for target, outs in stream:  # :1558-1571
            dst = sy.emitters[target]
            self.emit(sy, dst, dst.p.init_emit_count, F(0), sy.total_time, outs)

    # ---- ParticleSystem::update(dt) ------------------------------------------------------------------------------------------------
    def step(self, dt):
        self.step_no += 1
        dt = F(dt)
        for sy in self.systems:
            sy.sysv[:] = [dt, sy.total_time, 0, 0, F(sy.pos[0]), F(sy.pos[1]), F(sy.pos[2])]
            if sy.total_time == 0:
                for em in sy.emitters:
                    if em.p.emit_inputs == 0: self.emit(sy, em, em.p.init_emit_count, F(0), sy.total_time)
            sy.total_time = F(sy.total_time + dt)
            sy.sysv[A.TOTAL_TIME] = sy.total_time
            for em in sy.emitters:
                self.update_emitter(sy, em, dt)

    # ---- Emitter::fillInstanceData ---------------------------------------------------------------------------------------------------
    def fill(self):
        """[(slice of ((count + 3) & ~3) * outputs floats, count)] per emitter, in global emitter order"""
        res = []
        for sy in self.systems:
            for em in sy.emitters:
                out = np.zeros(((em.count + 3) & ~3) * em.p.outputs, F)
                for frm in range(0, em.count, CHUNK):
                    self.process_chunk(sy, em, frm, min(frm + CHUNK, em.count), em.p.output_offset, out, None)
                res.append((out, em.count))
        return res


def make_world(programs_by_system, capacities, seed=0, n_globals=0, positions=None):
    """programs_by_system: [[Program, ...], ...]; capacities likewise (or one int for all)."""
    systems = []
    for si, progs in enumerate(programs_by_system):
        ems = [Emitter(p, capacities if isinstance(capacities, int) else capacities[si][ei]) for ei, p in enumerate(progs)]
        systems.append(System(ems, n_globals, positions[si] if positions is not None else (0.0, 0.0, 0.0)))
    w = World(systems, seed)
    for s in systems:
        for e in s.emitters:
            w.prescan_rands(e)
    return w
