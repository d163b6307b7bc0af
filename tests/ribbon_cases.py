"""Ribbon scripts that stay where the reference is sound (max_len <= 1024, no KILL or EMIT, RIBBON_INDEX read only in emit programs, no
RAND): tests/test_ribbon_oracle_vs_ref.py holds the oracle to the sliced reference on them, tests/golden/make_golden_ribbons.py records
the reference's results for them, and tests/test_gpu_ribbons.py holds the device to that record.

A script is (systems, options, capacities, ops); an op is ("step", dt), ("emit_ribbons", system, emitter, n), ("kill", system, emitter,
ribbon) or ("move", [positions])."""
from tests import particle_asm as A
from tests import ribbon_oracle as R
from tests.particle_asm import CH, REG, LIT, SYS, OUT

EMIT = [A.mov(CH(0), SYS(A.EMIT_INDEX)), A.mov(CH(1), SYS(A.TOTAL_TIME)), A.mov(CH(2), SYS(A.RIBBON_INDEX)), A.mov(CH(3), LIT(0.0)), A.mov(CH(4), LIT(0.0)),
        A.mov(CH(5), SYS(A.ENTITY_X))]  # every channel the update reads: the ring of a new ribbon holds what an earlier one left (unspecified)
UPDATE = [A.add(CH(3), CH(3), SYS(A.TIME_DELTA)), A.mov(REG(1), LIT(2.0)), A.mod(REG(0), CH(0), REG(1)), A.lt(REG(1), REG(0), LIT(0.5)),
          A.cmp_else(REG(1), [A.add(CH(4), CH(4), LIT(1.0))], [A.sub(CH(4), CH(4), CH(3))])]
OUTPUT = [A.mov(OUT(0), CH(0)), A.madd(OUT(1), CH(3), LIT(2.0), CH(1)), A.mov(OUT(2), CH(2))]
SPRITE = A.Program([A.add(CH(1), CH(1), SYS(A.TIME_DELTA))], [A.mov(CH(0), SYS(A.ENTITY_X)), A.mov(CH(1), SYS(A.TOTAL_TIME))], [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1))],
                   channels=2, outputs=2)


def trail(init_emit_count=0, rate=0.0, emit=EMIT):
    return A.Program(UPDATE, emit, OUTPUT, channels=6, registers=2, outputs=3, init_emit_count=init_emit_count, emit_per_second=rate)


def steps(n, dt):
    return [("step", dt)] * n


CASES = {
    # max_len 8, 3 points a step for 6 steps: growth, saturation, offset advancing; one ribbon, so the reference's own fill is the packed one
    "ring": ([[trail(rate=30.0)]], [[R.Options(1, 8, 1)]], 16, steps(6, 0.105)),
    # two ribbons that fill up together: from the third step on every ribbon but the last is full
    "ring_two": ([[trail(rate=30.0)]], [[R.Options(2, 8, 2)]], 16, steps(5, 0.105)),
    # 20 points in one call into 8 slots, each reading what the one before left in its slot
    "order": ([[trail(init_emit_count=20, emit=[A.add(CH(0), CH(0), LIT(1.0)), A.mov(CH(1), SYS(A.EMIT_INDEX))])]], [[R.Options(1, 8, 1)]], 16, steps(1, 0.1)),
    # 30 a second, 5 points in a step into three ribbons: TOTAL_TIME is the repeated sum, restarted per ribbon
    "total_time": ([[trail(rate=30.0)]], [[R.Options(3, 8, 3)]], 16, steps(2, 0.17)),
    # unequal lengths 8, 5, 2 with three outputs; then the middle ribbon killed, a step, a new ribbon, a step; the last ribbon killed
    "unequal_kill": ([[trail(init_emit_count=2, rate=30.0)]], [[R.Options(3, 8, 1)]], 16,
                     [("step", 0.105), ("emit_ribbons", 0, 0, 1), ("step", 0.105), ("emit_ribbons", 0, 0, 1), ("kill", 0, 0, 1), ("step", 0.04), ("emit_ribbons", 0, 0, 1),
                      ("step", 0.04), ("kill", 0, 0, 5), ("kill", 0, 0, 2), ("step", 0.04)]),
    # emit_move_distance 4 against squared lengths 3.61 and 4.41; a ribbon and a non-ribbon emitter each gain exactly one; <= 0 emits nothing
    "movement": ([[trail(), SPRITE, trail(), SPRITE]],
                 [[R.Options(2, 12, 2, emit_move_distance=4.0), R.Options(emit_move_distance=4.0), R.Options(2, 12, 2, emit_move_distance=-1.0), R.Options(emit_move_distance=0.0)]], 16,
                 [("step", 0.1), ("move", [(1.9, 0.0, 0.0)]), ("move", [(0.0, 2.1, 0.0)]), ("move", [(0.0, 2.1, 1.9)]), ("step", 0.1), ("move", [(0.0, 2.1, 2.2)]), ("step", 0.1)]),
}
GOLDEN = ("ring", "order", "total_time", "unequal_kill", "movement")


def run_oracle(case):
    """The oracle over a script: [per op: [per emitter: (count, emit_index, records, live points [channels, n], packed slice rows)]]"""
    systems, options, capacities, ops = CASES[case]
    w = R.make_world(systems, capacities, options)
    trace = []
    for op in ops:
        if op[0] == "step": w.step(op[1])
        elif op[0] == "emit_ribbons": w.emit_ribbons(*op[1:])
        elif op[0] == "kill": w.kill_ribbon(*op[1:])
        else: w.apply_transforms(op[1])
        fills, state, g = w.fill(), [], 0
        for sy in w.systems:
            for em in sy.emitters:
                live = em.live() if em.is_ribbon else em.ch[:, :em.count]
                state.append((em.count, em.emit_index, em.records() if em.is_ribbon else [], live.copy(), fills[g][0][:em.count * em.p.outputs].copy()))
                g += 1
        trace.append(state)
    return trace
