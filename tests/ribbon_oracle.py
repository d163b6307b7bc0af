"""CPU oracle of the ribbon emitters: a plain-Python / numpy restatement of ParticleSystem::emitRibbonPoints, updateRibbons, emitRibbons,
killRibbon, applyTransform and the ribbon side of Emitter::fillInstanceData (renderer/particle_system.cpp), on top of the particle VM of
tests/particle_oracle.py.

The channels are kept in the reference's layout: ribbon r's ring at [r * max_len, (r + 1) * max_len) of every channel, killRibbon moves the
rings above the killed one down. The deviations of DESIGN.md §4.15.1 are stated where they apply:
  a. the slice is packed per ribbon: ribbon r's rows are its ring slots 0 .. length - 1, from row sum(length_q, q < r);
  b. RIBBON_INDEX reads the lane's own ribbon index in the emit, update and output programs of a ribbon emitter, 0 elsewhere;
  c. a reset system has no ribbons (the reference's reset() keeps them next to a particles_count of 0);
  d. last_emit_point starts at the origin (the reference gives it no initial value).
RAND keeps deviation 5's keying with ribbon * max_len + ring slot as the particle slot, which is the reference's particle index.
"""
import math

import numpy as np

from tests import particle_asm as A
from tests import particle_oracle as O

F = np.float32
U32 = 0xFFFFFFFF


class Options:
    """ParticleSystemResource::Emitter's fields next to the program (LmxParticleEmitterOptions)"""

    def __init__(self, max_ribbons=0, max_ribbon_length=0, init_ribbons_count=0, tube_segments=0, emit_move_distance=0.0):
        self.max_ribbons, self.init_ribbons_count, self.tube_segments = max_ribbons, init_ribbons_count, tube_segments
        self.max_ribbon_length = (max_ribbon_length + 3) & ~3  # particle_system.cpp:189
        self.emit_move_distance = F(emit_move_distance)

    def set_on(self, ps, system, emitter):
        ps.setEmitterOptions(system, emitter, self.max_ribbons, self.max_ribbon_length, self.init_ribbons_count, self.tube_segments, float(self.emit_move_distance))


class Ribbon:
    def __init__(self):
        self.offset = self.length = self.emit_index = 0


class Emitter(O.Emitter):
    def __init__(self, prog, capacity, opts=None):
        self.opts = opts or Options()
        if self.opts.max_ribbons:
            capacity = self.opts.max_ribbons * self.opts.max_ribbon_length
        super().__init__(prog, capacity)
        self.ribbons = []
        self.last_emit_point = (0.0, 0.0, 0.0)  # deviation d

    @property
    def is_ribbon(self):
        return self.opts.max_ribbons > 0

    def records(self):
        """[(offset, length, emit_index, points_offset)] per ribbon: what lmx_particles_ribbons answers"""
        out, row = [], 0
        for rb in self.ribbons:
            out.append((rb.offset, rb.length, rb.emit_index, row * self.p.outputs * 4))
            row += rb.length
        return out

    def live(self):
        """[channels, sum of lengths]: the live points of every ribbon, ring slots 0 .. length - 1, ribbon after ribbon"""
        L = self.opts.max_ribbon_length
        cols = [np.arange(r * L, r * L + rb.length) for r, rb in enumerate(self.ribbons)]
        return self.ch[:, np.concatenate(cols) if cols else np.zeros(0, np.int64)]


class World(O.World):
    # ---- ParticleSystem::emitRibbonPoints (:358-409) -----------------------------------------------------------------------------------
    def emit_ribbon_points(self, sy, em, r, count, time_step, c1):
        L = em.opts.max_ribbon_length
        rb = em.ribbons[r]
        regs = np.zeros((16, 1), F)
        t = F(c1)
        sy.sysv[A.RIBBON_INDEX] = F(r)
        for _ in range(count):
            if rb.length < L:
                rb.length += 1
                em.count += 1
            else:
                rb.offset = (rb.offset + 1) & U32
            slot = ((rb.offset + rb.length - 1) & U32) % L
            regs[:] = 0
            self.run(sy, em, em.p.emit_offset, r * L + slot, regs, 0, None, True, t, F(rb.emit_index))
            rb.emit_index = (rb.emit_index + 1) & U32
            t = F(t + F(time_step))
        sy.sysv[A.RIBBON_INDEX] = F(0)  # deviation b

    # ---- ParticleSystem::emitRibbons (:1597-1618) --------------------------------------------------------------------------------------
    def _emit_ribbons(self, sy, em, n, c1):
        n = min(n, em.opts.max_ribbons - len(em.ribbons))
        for _ in range(n):
            em.ribbons.append(Ribbon())
            self.emit_ribbon_points(sy, em, len(em.ribbons) - 1, em.p.init_emit_count, F(0), c1)

    def emit_ribbons(self, si, ei, n):
        """between steps: TOTAL_TIME and TIME_DELTA are what the last step left, the entity is where it is now"""
        sy = self.systems[si]
        em = sy.emitters[ei]
        if not em.is_ribbon: return
        sy.sysv[A.ENTITY_X:A.ENTITY_Z + 1] = [F(x) for x in sy.pos]
        self._emit_ribbons(sy, em, n, sy.sysv[A.TOTAL_TIME])

    # ---- ParticleSystem::killRibbon (:1574-1595) ---------------------------------------------------------------------------------------
    def kill_ribbon(self, si, ei, r):
        em = self.systems[si].emitters[ei]
        if r >= len(em.ribbons): return
        L = em.opts.max_ribbon_length
        n = (len(em.ribbons) - r - 1) * L
        if n > 0:
            em.ch[:, r * L:r * L + n] = em.ch[:, (r + 1) * L:(r + 1) * L + n].copy()
        em.count -= em.ribbons.pop(r).length

    # ---- ParticleSystem::applyTransform (:1377-1403), positions only -------------------------------------------------------------------
    def apply_transforms(self, positions):
        for sy, pos in zip(self.systems, positions):
            pos = tuple(float(x) for x in pos)
            sy.pos = pos
            sy.sysv[A.ENTITY_X:A.ENTITY_Z + 1] = [F(x) for x in pos]
            sy.sysv[A.TOTAL_TIME] = sy.total_time
            for em in sy.emitters:
                dist = em.opts.emit_move_distance
                if not dist > 0: continue
                d = [pos[k] - em.last_emit_point[k] for k in range(3)]
                if not d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > float(dist): continue  # a squared length against an unsquared distance
                em.last_emit_point = pos
                if em.is_ribbon:
                    for r in range(len(em.ribbons)): self.emit_ribbon_points(sy, em, r, 1, F(0), sy.total_time)
                else:
                    self.emit(sy, em, 1, F(0), sy.total_time)

    # ---- ParticleSystem::updateRibbons (:1405-1454) ------------------------------------------------------------------------------------
    def update_ribbons(self, sy, em, dt):
        p = em.p
        if p.emit_per_second > 0:
            em.emit_timer = F(em.emit_timer + F(dt))
            if em.emit_timer > 0:
                d = F(F(1) / F(p.emit_per_second))
                count = int(math.floor(float(F(em.emit_timer / d))))
                for r in range(len(em.ribbons)): self.emit_ribbon_points(sy, em, r, count, d, sy.total_time)
                em.emit_timer = F(em.emit_timer - F(d * F(count)))
        L = em.opts.max_ribbon_length
        for r, rb in enumerate(em.ribbons):  # ring slots [0, length): the chunk does not follow `offset`
            if rb.length == 0: continue
            sy.sysv[A.RIBBON_INDEX] = F(r)
            self.process_chunk(sy, em, r * L, r * L + rb.length, 0, None, {})
        sy.sysv[A.RIBBON_INDEX] = F(0)

    def step(self, dt):
        self.step_no += 1
        dt = F(dt)
        for sy in self.systems:
            sy.sysv[:] = [dt, sy.total_time, 0, 0, F(sy.pos[0]), F(sy.pos[1]), F(sy.pos[2])]
            if sy.total_time == 0:
                for em in sy.emitters:
                    if em.is_ribbon: self._emit_ribbons(sy, em, em.opts.init_ribbons_count, sy.total_time)
                    elif em.p.emit_inputs == 0: self.emit(sy, em, em.p.init_emit_count, F(0), sy.total_time)
            sy.total_time = F(sy.total_time + dt)
            sy.sysv[A.TOTAL_TIME] = sy.total_time
            for em in sy.emitters:
                if em.is_ribbon: self.update_ribbons(sy, em, dt)
                else: self.update_emitter(sy, em, dt)

    def reset(self, si=None):
        for k, sy in enumerate(self.systems):
            if si is not None and k != si: continue
            sy.total_time = F(0)
            for em in sy.emitters:
                em.count = em.emit_index = em.overflow = em.killed = 0
                em.emit_timer = F(0)
                em.ribbons = []  # deviation c

    # ---- Emitter::fillInstanceData, packed per ribbon (deviation a) ----------------------------------------------------------------------
    def fill_ribbons(self, sy, em):
        L, nout = em.opts.max_ribbon_length, em.p.outputs
        out = np.zeros(((em.count + 3) & ~3) * nout, F)
        row = 0
        for r, rb in enumerate(em.ribbons):
            if rb.length == 0: continue
            tmp = np.zeros((r * L + ((rb.length + 3) & ~3)) * nout, F)  # rows by particle index, as processChunk addresses them
            sy.sysv[A.RIBBON_INDEX] = F(r)
            self.process_chunk(sy, em, r * L, r * L + rb.length, em.p.output_offset, tmp, None)
            out[row * nout:(row + rb.length) * nout] = tmp[r * L * nout:(r * L + rb.length) * nout]
            row += rb.length
        sy.sysv[A.RIBBON_INDEX] = F(0)
        return out, em.count

    def fill(self):
        res = []
        for sy in self.systems:
            for em in sy.emitters:
                if em.is_ribbon:
                    res.append(self.fill_ribbons(sy, em))
                    continue
                out = np.zeros(((em.count + 3) & ~3) * em.p.outputs, F)
                for frm in range(0, em.count, O.CHUNK):
                    self.process_chunk(sy, em, frm, min(frm + O.CHUNK, em.count), em.p.output_offset, out, None)
                res.append((out, em.count))
        return res


def make_world(programs_by_system, capacities, options=None, seed=0, n_globals=0, positions=None):
    """programs_by_system: [[Program, ...], ...]; capacities and options likewise (capacities: or one int for all; options: None = none)."""
    systems = []
    for si, progs in enumerate(programs_by_system):
        ems = [Emitter(p, capacities if isinstance(capacities, int) else capacities[si][ei], options[si][ei] if options is not None else None) for ei, p in enumerate(progs)]
        systems.append(O.System(ems, n_globals, tuple(positions[si]) if positions is not None else (0.0, 0.0, 0.0)))
    w = World(systems, seed)
    for s in systems:
        for e in s.emitters:
            w.prescan_rands(e)
    return w
