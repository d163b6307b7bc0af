"""Particle systems on the device (lmx_particles_*) against tests/particle_oracle.py: every channel value in [0, count), every count and
every slice row in [0, count) bit for bit, the guards behind every channel and behind the frame buffer untouched."""
import struct

import numpy as np
import pytest

from tests import particle_asm as A
from tests import particle_oracle as O
from tests.conftest import hostsim_active
from tests.particle_asm import CH, REG, LIT, LIT_BITS, SYS, GLOB, OUT

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g, w = u32(got), u32(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: got {int(g[tuple(bad[0])]):#010x}, want {int(w[tuple(bad[0])]):#010x}")


class Pair:
    """The device object and the oracle world over the same programs."""

    def __init__(self, ctx, systems, capacities, seed=0, globals_=None, positions=None):
        from lumixengine_amd import api

        self.ps = api.ParticleSystems(ctx)
        ng = len(globals_) if globals_ is not None else 0
        self.world = O.make_world(systems, capacities, seed, ng, positions)
        self.systems = systems
        for si, progs in enumerate(systems):
            assert self.ps.addSystem(len(progs), ng) == si
            if ng:
                self.ps.setGlobals(si, globals_)
                self.world.systems[si].globals[:] = globals_
            for ei, p in enumerate(progs):
                p.set_on(self.ps, si, ei)
                self.ps.reserve(si, ei, capacities if isinstance(capacities, int) else capacities[si][ei])
        if positions is not None:
            self.ps.setEntityPositions(positions)
        self.ps.setSeed(seed)

    def step(self, dt, check=True):
        self.ps.update(dt)
        self.ps.fill()
        self.world.step(dt)
        if check:
            self.check()

    def check(self):
        counts = self.ps.counts()
        slices, frame = self.ps.readSlices()
        want = self.world.fill()
        offset, g = 0, 0
        for si, sy in enumerate(self.world.systems):
            for ei, em in enumerate(sy.emitters):
                c = counts[g]
                assert (int(c["particles"]), int(c["emit_index"]), int(c["overflow"]), int(c["killed"])) == (em.count, em.emit_index, em.overflow, em.killed), (si, ei)
                got = self.ps.readChannels(si, ei, em.p.channels)
                assert_bits(got[:, :em.count], em.ch[:, :em.count], f"channels of system {si} emitter {ei}")
                assert np.all(u32(got[:, em.capacity:]) == GUARD), (si, ei, "channel guard written")
                out, n = want[g]
                s = slices[g]
                assert (int(s["offset"]), int(s["bytes"]), int(s["particles"])) == (offset, out.nbytes, n), (si, ei)
                assert offset % 16 == 0
                rows = frame[offset // 4: offset // 4 + n * em.p.outputs]
                assert_bits(rows, out[:n * em.p.outputs], f"slice of system {si} emitter {ei}")
                offset += out.nbytes
                g += 1
        assert np.all(u32(frame[-64:]) == GUARD), "frame guard written"

    def close(self):
        self.ps.close()


def run(ctx, systems, capacities, dts, **kw):
    p = Pair(ctx, systems, capacities, **kw)
    try:
        for dt in dts:
            p.step(dt)
    finally:
        p.close()
    return p


def table(dst, values, r0=REG(0), r1=REG(1)):
    """emit-program instructions: dst = values[EMIT_INDEX] (bit patterns), left alone for other indices"""
    body = []
    for i, v in enumerate(values):
        lit = LIT_BITS(v) if isinstance(v, int) else LIT(v)
        body += [A.sub(r0, SYS(A.EMIT_INDEX), LIT(float(i))), A.not_(r1, r0), A.cmp(r1, [A.mov(dst, lit)])]
    return body


ID_EMIT = [A.mov(CH(0), SYS(A.EMIT_INDEX)), A.mov(CH(1), LIT(0.0)), A.mov(CH(2), LIT(3.0))]


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4097, 5 * 1024 + 1])
def test_counts(gpu_ctx, n):
    """n particles, every third killed in the first step and again in the second: chunks, the padded four, compaction across chunks."""
    update = [A.add(CH(1), CH(1), SYS(A.TIME_DELTA)), A.mod(REG(0), CH(0), CH(2)), A.lt(REG(1), REG(0), LIT(0.5)), A.cmp(REG(1), [A.KILL])]
    output = [A.mov(OUT(0), CH(0)), A.mul(OUT(1), CH(1), LIT(2.0))]
    p = A.Program(update, ID_EMIT, output, channels=3, registers=2, outputs=2, init_emit_count=n)
    run(gpu_ctx, [[p]], n + 1, [0.25, 0.5])


# ---- instructions ----------------------------------------------------------------------------------------------------------------------
SPECIAL = [0.0, 1.0, -1.0, 0.5, -2.75, 3.0, 1.0e6, -1.0e-3, 0x7FC00000, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000, 7.25, 100.0, -100.0, 4294967296.0,
           4294967040.0, 4294967808.0, -4294967296.0, 2.0, -0.5, 1.0e20, -1.0e20, 0x00000001]


def special_emit(nch=3):
    """channel 0 = the particle's index, channel 1 = SPECIAL[index], channel 2 = SPECIAL rotated by seven"""
    return [A.mov(CH(0), SYS(A.EMIT_INDEX))] + table(CH(1), SPECIAL) + table(CH(2), SPECIAL[7:] + SPECIAL[:7])


def test_whole_chunk_instructions(gpu_ctx):
    """Every whole-chunk instruction, each operand kind in each position the decoder accepts; DIV and MOD by zero and of NaN, MIN / MAX with
    NaN in either operand, gnoise at negative, zero, integer and 2^32 +- 1 ulp arguments."""
    n = len(SPECIAL)
    two = [A.add, A.sub, A.mul, A.div, A.max_, A.min_, A.lt, A.gt, A.and_, A.or_]

    def binary(ops, time):
        """per instruction: channel x channel -> channel; channel x literal -> register; system value x register -> register; global x register -> channel"""
        out, k = [], 3
        for f in ops:
            out += [f(CH(k), CH(1), CH(2)), f(REG(0), CH(1), LIT(2.5)), f(REG(1), SYS(time), REG(0)), f(CH(k + 1), GLOB(1), REG(1))]
            k += 2
        return out

    # the first six binary instructions, and in the output program: channel x channel -> output, literal x global -> output
    output = []
    for i, f in enumerate(two[:6]):
        output += [f(OUT(2 * i), CH(3 + 2 * i), CH(4 + 2 * i)), f(OUT(2 * i + 1), LIT(-1.5), GLOB(0))]
    p1 = A.Program(binary(two[:6], A.TIME_DELTA), special_emit(), output + [A.mov(OUT(12), CH(1))], channels=16, registers=2, outputs=13, init_emit_count=n)
    # the other four, then the rest
    upd2 = binary(two[6:], A.TOTAL_TIME)
    upd2 += [A.mod(CH(11), CH(1), CH(2)), A.mod(REG(2), CH(2), CH(1)), A.sqrt(CH(12), CH(1)), A.sqrt(REG(3), REG(2)), A.noise(CH(13), CH(1)), A.noise(REG(4), CH(2)),
             A.mov(REG(6), LIT(4.5)), A.madd(CH(14), CH(1), LIT(3.0), REG(6)), A.mix(CH(15), CH(1), CH(2), LIT(0.3)), A.lt(REG(5), CH(1), CH(2)), A.blend(CH(3), CH(1), CH(2), REG(5)),
             A.mov(REG(6), LIT(4.5)), A.mov(REG(7), SYS(A.ENTITY_Y)), A.mov(CH(4), REG(7)), A.mov(CH(5), CH(1)),
             A.gradient(REG(8), CH(1), [0.0, 3.0], [1.0, -1.0]), A.mov(CH(6), REG(8))]
    out2 = [A.mov(OUT(0), GLOB(0)), A.mov(OUT(1), LIT(9.0)), A.mov(OUT(2), CH(3)), A.mov(REG(0), CH(11)), A.mov(OUT(3), REG(0)), A.noise(OUT(4), CH(1)), A.sqrt(OUT(5), CH(12)),
            A.mod(OUT(6), CH(1), CH(2)), A.madd(OUT(7), CH(13), GLOB(1), SYS(A.ENTITY_X)), A.mix(OUT(8), LIT(1.0), CH(14), CH(15)), A.blend(OUT(9), CH(1), CH(2), CH(1)),
             A.gradient(OUT(10), CH(1), [-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 3.0, 7.25], [0.0, 1.0, 0.5, 4.0, -4.0, 2.0, 8.0, 1.0]), A.mov(OUT(11), CH(6)),
             A.gradient(OUT(12), CH(2), [0.0, 3.0], [1.0, -1.0])]
    p3 = A.Program(upd2, special_emit(), out2, channels=16, registers=9, outputs=13, init_emit_count=n)
    run(gpu_ctx, [[p1, p3]], n + 3, [0.125, 0.25], globals_=[0.75, -3.0], positions=[(1.0e6 + 0.3, -2.5, 7.0)])


def test_block_instructions(gpu_ctx):
    """Every instruction the scalar interpreter runs, inside conditional blocks (an emitter of <= 1024 particles: registers are chunk-local),
    with each operand kind, nested CMP / CMP_ELSE, and the output program's blocks reading and writing outputs."""
    n = len(SPECIAL)
    two = [A.add, A.sub, A.mul, A.div, A.mod, A.max_, A.min_, A.lt, A.gt, A.and_, A.or_]
    body = []
    for i, f in enumerate(two):
        body += [f(REG(2), CH(1), CH(2)), f(REG(3), REG(2), LIT(2.5)), f(CH(3 + i), SYS(A.TIME_DELTA), REG(3))]
    body += [A.not_(REG(4), CH(1)), A.mov(CH(14), REG(4)), A.madd(CH(15), CH(1), GLOB(1), LIT(0.5)), A.mix(REG(5), CH(1), CH(2), GLOB(0)), A.sqrt(REG(6), CH(2)),
             A.noise(REG(7), CH(0)), A.max_(REG(5), REG(5), REG(6)), A.add(CH(2), REG(5), REG(7)),
             A.cmp(CH(1), [A.mov(CH(1), LIT(0.0)), A.cmp_else(REG(4), [A.mov(CH(0), LIT(-1.0))], [A.cmp(CH(2), [A.add(CH(0), CH(0), LIT(100.0))])])])]
    update = [A.gt(REG(0), CH(0), LIT(1.5)), A.lt(REG(1), CH(0), LIT(3.5)), A.cmp(REG(0), body), A.cmp_else(REG(1), [A.mov(CH(13), LIT(1.0))], [A.mov(CH(13), LIT(2.0))])]
    output = [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(2)), A.lt(REG(0), CH(0), LIT(10.0)),
              A.cmp_else(REG(0), [A.add(OUT(2), OUT(0), OUT(1)), A.mov(REG(1), OUT(2)), A.mul(OUT(3), REG(1), SYS(A.TOTAL_TIME))], [A.mov(OUT(2), GLOB(0)), A.mov(OUT(3), CH(15))])]
    p = A.Program(update, special_emit(), output, channels=16, registers=8, outputs=4, init_emit_count=n)
    run(gpu_ctx, [[p]], n + 2, [0.125, 0.25], globals_=[0.75, -3.0])


# ---- kills -----------------------------------------------------------------------------------------------------------------------------
def kill_program(n, pred, body=(A.KILL,), els=None, channels=3, extra=()):
    """pred: whole-chunk instructions that leave the mask in REG(1)"""
    blk = A.cmp(REG(1), list(body)) if els is None else A.cmp_else(REG(1), list(body), list(els))
    update = [A.add(CH(1), CH(1), SYS(A.TIME_DELTA))] + list(pred) + [blk] + list(extra)
    return A.Program(update, ID_EMIT, [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1))], channels=channels, registers=3, outputs=2, init_emit_count=n)


def below(x): return [A.lt(REG(1), CH(0), LIT(x))]
def above(x): return [A.gt(REG(1), CH(0), LIT(x))]
def between(a, b): return [A.gt(REG(0), CH(0), LIT(a)), A.lt(REG(1), CH(0), LIT(b)), A.and_(REG(1), REG(0), REG(1))]
EVERY_OTHER = [A.mov(REG(2), LIT(2.0)), A.mod(REG(0), CH(0), REG(2)), A.lt(REG(1), REG(0), LIT(0.5))]


KILL_CASES = {
    "none": (1500, below(-1.0)),
    "all": (1500, above(-1.0)),
    "first": (1500, below(0.5)),
    "last": (1500, above(1498.5)),
    "every_other": (2100, EVERY_OTHER),
    "last_k_of_chunk": (2048, between(1023.5 - 17, 1023.5)),
    "tail_fewer_survivors": (1024 + 30, between(99.5, 199.5)),   # 100 kills in the head chunk, 30 particles in the tail
    "tail_more_survivors": (1024 + 300, between(99.5, 199.5)),
    "three_chunks": (3 * 1024 + 5, between(10.5, 1500.5)),
}


@pytest.mark.parametrize("case", sorted(KILL_CASES))
def test_kills(gpu_ctx, case):
    n, pred = KILL_CASES[case]
    run(gpu_ctx, [[kill_program(n, pred)]], n, [0.5, 0.25])


def test_kill_in_the_padded_four(gpu_ctx):
    """CMP_ELSE runs its false arm on the rows between count and the next multiple of four: their kills count and move `last`."""
    run(gpu_ctx, [[kill_program(5, above(-1.0), body=[A.mov(CH(1), LIT(7.0))], els=[A.KILL])]], 8, [0.5, 0.25])
    run(gpu_ctx, [[kill_program(1029, above(-1.0), body=[A.mov(CH(1), LIT(7.0))], els=[A.KILL])]], 1032, [0.5, 0.25])


def test_two_blocks_that_kill(gpu_ctx):
    """The second block starts again from last = to - 1 and overwrites the chunk's kill count."""
    second = [A.gt(REG(1), CH(0), LIT(40.5)), A.cmp(REG(1), [A.KILL])]
    for n in (70, 1100):
        run(gpu_ctx, [[kill_program(n, below(9.5), extra=second)]], n, [0.5, 0.25])


def test_cmp_else_kills_in_the_false_arm(gpu_ctx):
    for n in (64, 1300):
        run(gpu_ctx, [[kill_program(n, EVERY_OTHER, body=[A.add(CH(1), CH(1), LIT(1.0))], els=[A.mov(CH(2), LIT(5.0)), A.KILL])]], n, [0.5, 0.25])


def test_block_writes_a_channel_and_then_kills(gpu_ctx):
    """A killed slot takes the values of `last` from BEFORE the block ran there when the loop has not reached it, from after when it has.
    (The block keeps its conditions in a channel: registers inside blocks are for emitters of one chunk, DESIGN §4.15 deviation 3.)"""
    body = [A.add(CH(1), CH(1), LIT(10.0)), A.mul(CH(2), CH(0), LIT(2.0)), A.lt(CH(3), CH(0), LIT(20.5)), A.cmp(CH(3), [A.KILL]), A.gt(CH(3), CH(0), LIT(55.5)), A.cmp(CH(3), [A.KILL])]
    for n in (64, 70, 1500):
        run(gpu_ctx, [[kill_program(n, above(-1.0), body=body, channels=4)]], n, [0.5, 0.25, 0.125])


# ---- emission --------------------------------------------------------------------------------------------------------------------------
TIME_EMIT = [A.mov(CH(0), SYS(A.EMIT_INDEX)), A.mov(CH(1), SYS(A.TOTAL_TIME)), A.add(CH(2), SYS(A.ENTITY_X), SYS(A.TIME_DELTA))]
AGE = [A.add(CH(2), CH(2), SYS(A.TIME_DELTA))]
OUT3 = [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1)), A.mov(OUT(2), CH(2))]


def test_init_emit_count_on_the_first_step_only(gpu_ctx):
    p = A.Program(AGE, TIME_EMIT, OUT3, channels=3, outputs=3, init_emit_count=37)
    run(gpu_ctx, [[p]], 64, [0.1, 0.1, 0.1], positions=[(4.0, 5.0, 6.0)])


@pytest.mark.parametrize("dt", [0.004, 0.01, 0.025, 0.3])
def test_emit_per_second(gpu_ctx, dt):
    """100 particles a second with dt below, at and above one period; 0.3 s at 10000 a second is 3000 in one step: TOTAL_TIME of the i-th is
    the repeated fp32 sum."""
    rate = 10000.0 if dt == 0.3 else 100.0
    p = A.Program(AGE, TIME_EMIT, OUT3, channels=3, outputs=3, init_emit_count=2, emit_per_second=rate)
    run(gpu_ctx, [[p]], 3100 * 3 if dt == 0.3 else 64, [dt, dt, dt])


@pytest.mark.parametrize("n", [39, 40, 41])
def test_emission_at_capacity(gpu_ctx, n):
    """capacity - 1, capacity and capacity + 1 particles into a capacity of 40: past it they are counted, not written, and the overflow bit is set."""
    p = A.Program(AGE, TIME_EMIT, OUT3, channels=3, outputs=3, init_emit_count=n)
    pair = run(gpu_ctx, [[p]], 40, [0.1, 0.1])
    em = pair.world.systems[0].emitters[0]
    assert em.overflow == (1 if n == 41 else 0) and em.count == min(n, 40) and em.emit_index == n


def test_overflow_over_several_chunks(gpu_ctx):
    p = A.Program(AGE, TIME_EMIT, OUT3, channels=3, outputs=3, init_emit_count=1030, emit_per_second=1000.0)
    pair = run(gpu_ctx, [[p]], 1100, [0.05, 0.05, 0.05])
    assert pair.world.systems[0].emitters[0].overflow == 1


# ---- sub-emission ------------------------------------------------------------------------------------------------------------------------
def spawner(n, target, pred, then_kill=True, extra_body=()):
    """n particles; those the predicate (mask in REG(1)) picks EMIT into `target` with outputs {index, 2 x index + TIME_DELTA} and die"""
    body = [A.emit(target, [A.mov(OUT(0), CH(0)), A.madd(OUT(1), CH(0), LIT(2.0), SYS(A.TIME_DELTA))])] + list(extra_body) + ([A.KILL] if then_kill else [])
    update = [A.add(CH(1), CH(1), SYS(A.TIME_DELTA))] + list(pred) + [A.cmp(REG(1), body)]
    return A.Program(update, ID_EMIT, [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1))], channels=3, registers=3, outputs=2, init_emit_count=n)


def receiver(per_record, update=(), emit_inputs=2):
    """what the records make: channel 0 = first input, 1 = second input + EMIT_INDEX, 2 = TOTAL_TIME"""
    emit = [A.mov(CH(0), REG(0)), A.add(CH(1), REG(1), SYS(A.EMIT_INDEX)), A.mov(CH(2), SYS(A.TOTAL_TIME)), A.mov(REG(2), LIT(1.0))]
    return A.Program(list(update) + AGE, emit, OUT3, channels=3, registers=3, outputs=3, emit_inputs=emit_inputs, init_emit_count=per_record)


@pytest.mark.parametrize("records", [0, 1, 1025])
def test_sub_emission_into_a_later_emitter(gpu_ctx, records):
    """0, 1 and 1025 records, three particles each, the emit inputs passed through: the later emitter updates them in the same step"""
    n = 2100
    pred = below(records - 0.5) if records <= 1 else between(99.5, 99.5 + records)
    run(gpu_ctx, [[spawner(n, 1, pred), receiver(3)]], [[n, 3 * 1025 + 8]], [0.5, 0.25])


def test_sub_emission_into_an_earlier_emitter(gpu_ctx):
    """the target has had its update: the new particles wait for the next step; a second system keeps its own targets"""
    sys0 = [receiver(2), spawner(70, 0, EVERY_OTHER)]
    sys1 = [receiver(1), spawner(1100, 0, between(1000.5, 1050.5), then_kill=False)]
    run(gpu_ctx, [sys0, sys1], [[200, 70], [400, 1100]], [0.5, 0.25, 0.125])


def chain_of_three():
    """emitter 0 spawns into 1, whose particles spawn twice into 2 when they have aged, and 2 spawns back into 0 or into 1: two EMITs in one
    block, EMITs in both arms of a CMP_ELSE"""
    first = spawner(40, 1, below(9.5))
    second = A.Program([A.add(CH(2), CH(2), LIT(1.0)), A.gt(REG(1), CH(2), LIT(1.5)),
                        A.cmp(REG(1), [A.emit(2, [A.mov(OUT(0), CH(1)), A.mov(OUT(1), CH(2))]), A.emit(2, [A.mov(OUT(1), LIT(-1.0))]), A.KILL])],
                       [A.mov(CH(0), REG(0)), A.mov(CH(1), REG(1)), A.mov(CH(2), LIT(0.0))], OUT3, channels=3, registers=2, outputs=3, emit_inputs=2, init_emit_count=2)
    third = receiver(1, update=[A.lt(REG(1), CH(0), LIT(25.0)), A.cmp_else(REG(1), [A.emit(0, [])], [A.emit(1, [A.mov(OUT(0), LIT(7.0))])]), A.mov(CH(0), LIT(99.0))])
    return [first, second, third]


@pytest.mark.parametrize("capacities", [[44, 64, 28], [8192, 8192, 8192]])
def test_sub_emission_chain_of_three(gpu_ctx, capacities):
    """with room for everything, and with capacities that run out on the way"""
    run(gpu_ctx, [chain_of_three()], [capacities], [0.5, 0.25, 0.125, 0.5, 0.25])


# ---- several systems ---------------------------------------------------------------------------------------------------------------------
def generated_program(rng):
    """a small seeded program: motion, an age, a death rule (no RAND)"""
    life = float(rng.uniform(0.3, 1.2))
    g = float(rng.uniform(-9.0, -1.0))
    emit = [A.mov(CH(0), SYS(A.ENTITY_X)), A.mul(CH(1), SYS(A.EMIT_INDEX), LIT(float(rng.uniform(0.1, 2.0)))), A.mov(CH(2), LIT(0.0)), A.mov(CH(3), SYS(A.TOTAL_TIME))]
    update = [A.madd(CH(1), SYS(A.TIME_DELTA), LIT(g), CH(1)), A.madd(CH(0), CH(1), SYS(A.TIME_DELTA), CH(0)), A.add(CH(2), CH(2), SYS(A.TIME_DELTA)),
              A.gt(REG(0), CH(2), LIT(life))]
    kind = int(rng.integers(3))
    if kind == 0: update += [A.cmp(REG(0), [A.KILL])]
    elif kind == 1: update += [A.cmp_else(REG(0), [A.KILL], [A.mix(CH(3), CH(3), CH(0), GLOB(0))])]
    else: update += [A.cmp(REG(0), [A.sub(CH(2), CH(2), LIT(life)), A.lt(REG(1), CH(1), LIT(g * 0.5)), A.cmp(REG(1), [A.KILL])])]
    output = [A.mov(OUT(0), CH(0)), A.mix(OUT(1), CH(1), CH(3), LIT(0.25)), A.div(OUT(2), CH(2), LIT(life))]
    return A.Program(update, emit, output, channels=4, registers=2, outputs=3, init_emit_count=int(rng.integers(0, 6)), emit_per_second=float(rng.choice([0.0, 7.0, 19.0, 40.0])))


def test_300_systems_of_3_emitters_for_20_steps(gpu_ctx):
    def make():
        rng = np.random.default_rng(17)
        systems = [[generated_program(rng) for _ in range(3)] for _ in range(300)]
        pos = rng.uniform(-50.0, 50.0, (300, 3))
        return Pair(gpu_ctx, systems, 48, globals_=[0.125], positions=pos)

    a = make()
    rng = np.random.default_rng(5)
    dts = [float(x) for x in rng.uniform(0.01, 0.12, 20)]
    trace = []
    for dt in dts:
        a.step(dt)
        trace.append((a.ps.counts().tobytes(), a.ps.readSlices()[1].tobytes()))
    assert sum(int(c["particles"]) for c in a.ps.counts()) > 1000 and sum(int(c["killed"]) for c in a.ps.counts()) > 0
    a.close()
    b = make()  # the same run again: identical bytes
    for dt, t in zip(dts, trace):
        b.step(dt, check=False)
        assert (b.ps.counts().tobytes(), b.ps.readSlices()[1].tobytes()) == t
    b.close()


# ---- RAND ------------------------------------------------------------------------------------------------------------------------------
def rand_pair(ctx, n, seed):
    emit = [A.rand(CH(0), -2.0, 3.0)]
    update = [A.rand(CH(1), 0.0, 1.0), A.rand(REG(0), 5.0, 6.0), A.mov(CH(2), REG(0)), A.gt(REG(1), CH(0), LIT(-5.0)), A.cmp(REG(1), [A.rand(CH(3), -1.0, 1.0)])]
    p = A.Program(update, emit, [A.rand(OUT(0), 10.0, 20.0), A.mov(OUT(1), CH(1))], channels=4, registers=2, outputs=2, init_emit_count=n)
    return Pair(ctx, [[p], [p]], n, seed=seed)


def test_rand(gpu_ctx):
    a = rand_pair(gpu_ctx, 1100, 1234)
    a.step(0.1)
    a.step(0.1)
    ch = a.ps.readChannels(0, 0, 4)[:, :1100]
    for row, (lo, hi) in zip(ch, [(-2.0, 3.0), (0.0, 1.0), (5.0, 6.0), (-1.0, 1.0)]):
        assert np.all(row >= lo) and np.all(row < hi)
        assert len(np.unique(row)) > 1000  # different particles differ
    other = a.ps.readChannels(1, 0, 4)[:, :1100]
    assert not np.array_equal(ch[1], other[1])  # ... and so do emitters
    first = ch.copy()
    a.step(0.1)
    assert not np.array_equal(a.ps.readChannels(0, 0, 4)[1, :1100], first[1])  # ... and steps
    frames = a.ps.readSlices()[1].tobytes()
    a.close()
    b = rand_pair(gpu_ctx, 1100, 1234)  # the same seed: the same bytes
    for _ in range(3):
        b.step(0.1, check=False)
    assert b.ps.readSlices()[1].tobytes() == frames
    b.close()
    c = rand_pair(gpu_ctx, 1100, 99)
    for _ in range(3):
        c.step(0.1, check=False)
    assert c.ps.readSlices()[1].tobytes() != frames
    c.close()


def test_rand_mean(gpu_ctx):
    """10^5 draws of [2, 6): the mean within 4 standard errors (4 / sqrt(12) / sqrt(n)) of the midpoint"""
    from lumixengine_amd import api

    n = 100000
    p = A.Program([], [A.rand(CH(0), 2.0, 6.0)], [A.mov(OUT(0), CH(0))], channels=1, outputs=1, init_emit_count=n)
    ps = api.ParticleSystems(gpu_ctx)
    ps.addSystem(1)
    p.set_on(ps, 0, 0)
    ps.reserve(0, 0, n)
    ps.setSeed(7)
    ps.update(0.1)
    v = ps.readChannels(0, 0, 1)[0, :n].astype(np.float64)
    ps.close()
    assert v.min() >= 2.0 and v.max() < 6.0
    assert abs(v.mean() - 4.0) <= 4.0 * (4.0 / np.sqrt(12.0)) / np.sqrt(n)


def test_rand_formula_is_the_references():
    """from + float((to - from) * (r * 2.328306435996595e-10)) with the double product, on the oracle's side of the comparison"""
    assert O.rand_float(0.0, 1.0, 0) == 0.0 and O.rand_float(0.0, 1.0, 0xFFFFFFFF) == np.float32(0xFFFFFFFF * 2.328306435996595e-10)
    assert O.rand_float(-2.0, 3.0, 0x80000000) == np.float32(-2.0) + np.float32(5.0 * (0x80000000 * 2.328306435996595e-10))


# ---- SIN / COS ---------------------------------------------------------------------------------------------------------------------------
SINCOS_ULP_BOUND = 2  # twice the largest distance measured on the MI355X over this argument set: 1 ulp; the cap is 4


def sincos_args():
    rng = np.random.default_rng(3)
    special = [0.0, np.pi, -np.pi, 2 * np.pi, np.pi / 2, -np.pi / 2, 3 * np.pi, 100 * np.pi, 1.0e6]
    return np.concatenate([rng.uniform(-100.0, 100.0, 4096), special]).astype(np.float32)


def ulp_distance(a, b):
    def key(x):
        u = u32(x).astype(np.int64)
        return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))


def test_sin_cos(gpu_ctx):
    """The result goes straight into a channel and an output, nothing downstream. Bit-equal on the simulated device (the same libm); on
    the GPU within SINCOS_ULP_BOUND ulps of the reference's libm result."""
    from lumixengine_amd import api

    args = sincos_args()
    n = len(args)
    # the arguments travel as globals, 256 per system: the emit program picks global EMIT_INDEX
    per = 256
    systems = []
    for s0 in range(0, n, per):
        m = min(per, n - s0)
        emit = [A.mov(CH(0), SYS(A.EMIT_INDEX))]
        for i in range(m):
            emit += [A.sub(REG(0), SYS(A.EMIT_INDEX), LIT(float(i))), A.not_(REG(1), REG(0)), A.cmp(REG(1), [A.mov(CH(0), GLOB(i))])]
        update = [A.sin(CH(1), CH(0)), A.cos(CH(2), CH(0)), A.gt(REG(0), CH(0), LIT(-1.0e9)), A.cmp(REG(0), [A.sin(CH(3), CH(0)), A.cos(CH(4), CH(0))])]
        output = [A.sin(OUT(0), CH(0)), A.cos(OUT(1), CH(0))]
        systems.append((A.Program(update, emit, output, channels=5, registers=2, outputs=2, init_emit_count=m), args[s0:s0 + m]))
    ps = api.ParticleSystems(gpu_ctx)
    for si, (p, g) in enumerate(systems):
        ps.addSystem(1, per)
        ps.setGlobals(si, np.concatenate([g, np.zeros(per - len(g), np.float32)]))
        p.set_on(ps, si, 0)
        ps.reserve(si, 0, per)
    ps.update(0.1)
    ps.fill()
    slices, frame = ps.readSlices()
    worst = 0
    for si, (p, g) in enumerate(systems):
        ch = ps.readChannels(si, 0, 5)[:, :len(g)]
        assert np.array_equal(u32(ch[0]), u32(g))
        want_s, want_c = O.vsinf(g), O.vcosf(g)
        rows = frame[slices[si]["offset"] // 4:][:2 * len(g)].reshape(-1, 2)
        for got, want in ((ch[1], want_s), (ch[2], want_c), (ch[3], want_s), (ch[4], want_c), (rows[:, 0], want_s), (rows[:, 1], want_c)):
            worst = max(worst, int(ulp_distance(got, want).max()))
    ps.close()
    print(f"SIN / COS: largest distance to libm {worst} ulp over {n} arguments")
    assert worst <= (0 if hostsim_active() else SINCOS_ULP_BOUND)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    import ctypes as C

    from lumixengine_amd import api

    lib = gpu_ctx.lib
    h = C.c_void_p()
    assert lib.lmx_particles_create(None, C.byref(h)) == 1
    assert lib.lmx_particles_create(gpu_ctx.h, None) == 1
    cnt = np.zeros(4, api.PARTICLES_COUNTS)
    prog = api.LmxParticleProgram()
    dev = api.LmxParticlesDevice()
    stride = C.c_uint32()
    for foreign in (None, gpu_ctx.h):  # a null object, and an object of another kind
        assert lib.lmx_particles_add_system(foreign, 1, 0, None) == 1
        assert lib.lmx_particles_set_program(foreign, 0, 0, C.byref(prog)) == 1
        assert lib.lmx_particles_set_globals(foreign, 0, None, 0) == 1
        assert lib.lmx_particles_set_entity_positions(foreign, 0, None) == 1
        assert lib.lmx_particles_reserve(foreign, 0, 0, 4) == 1
        assert lib.lmx_particles_reset(foreign, 0) == 1
        assert lib.lmx_particles_set_seed(foreign, 1) == 1
        assert lib.lmx_particles_step(foreign, 0.1) == 1
        assert lib.lmx_particles_fill(foreign) == 1
        assert lib.lmx_particles_counts(foreign, api._ptr(cnt), 4) == 1
        assert lib.lmx_particles_read_channels(foreign, 0, 0, None, 0, C.byref(stride)) == 1
        assert lib.lmx_particles_read_slices(foreign, None, 0, None, 0) == 1
        assert lib.lmx_particles_device_outputs(foreign, C.byref(dev)) == 1
        lib.lmx_particles_destroy(foreign)

    ps = api.ParticleSystems(gpu_ctx)
    ps.update(0.1)  # an empty world
    ps.fill()
    assert len(ps.counts()) == 0 and len(ps.readSlices()[0]) == 0
    ps.addSystem(2)
    ok = A.Program([], [A.mov(CH(0), LIT(1.0))], [A.mov(OUT(0), CH(0))], init_emit_count=3)
    ok.set_on(ps, 0, 0)
    with pytest.raises(api.LumixError) as e:  # a step before every program is set
        ps.update(0.1)
    assert e.value.code == 6
    for bad in (A.Program([A.gt(REG(0), CH(0), LIT(0.0)), A.cmp(REG(0), [A.mesh(CH(0), REG(0), 1)])], [], [], registers=1),
                A.Program([], [], [A.spline(OUT(0), CH(0), 2)])):
        with pytest.raises(api.LumixError) as e:
            bad.set_on(ps, 0, 1)
        assert e.value.code == 9
    with pytest.raises(api.LumixError) as e:
        A.Program([A.KILL], [], []).set_on(ps, 0, 1)
    assert e.value.code == 8
    for call in (lambda: ok.set_on(ps, 1, 0), lambda: ok.set_on(ps, 0, 2), lambda: ps.reserve(0, 2, 4), lambda: ps.reset(3), lambda: ps.setGlobals(0, [1.0]),
                 lambda: ps.setEntityPositions(np.zeros((2, 3)))):
        with pytest.raises(api.LumixError) as e:
            call()
        assert e.value.code == 1
    ok.set_on(ps, 0, 1)
    ps.reserve(0, 0, 8)
    ps.update(0.1)
    c = ps.counts()
    assert [int(x) for x in c["particles"]] == [3, 0] and int(c["overflow"][1]) == 1  # emitter 1 has no capacity
    ps.reset()
    assert [int(x) for x in ps.counts()["particles"]] == [0, 0]
    ps.close()
    # a system the engine keeps to itself (the adapter's answer to a refused program): empty programs, no capacity - the others go on
    ps = api.ParticleSystems(gpu_ctx)
    ps.addSystem(2)
    ps.addSystem(1)
    for e in range(2):
        ps.setProgram(0, e, bytes(3), 1, 2, 0, 0, 0)
        ps.reserve(0, e, 0)
    ok.set_on(ps, 1, 0)
    ps.reserve(1, 0, 8)
    ps.update(0.1)
    ps.fill()
    assert [int(x) for x in ps.counts()["particles"]] == [0, 0, 3] and not ps.counts()["overflow"].any()
    ps.close()
