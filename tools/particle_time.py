#!/usr/bin/env python
"""Times one particle step plus fill on the device: --emitters emitters (one per system) of --particles particles each, a 30-instruction
update program (motion under gravity and drag, a noise wobble, a colour gradient, an age test whose block kills) and a 12-float output
program. Median of --steps spans between stream events, warm (back to back) and behind a 1 GiB scrub of the caches; one JSON line with
the algorithmic bytes (4 B x channels read and written + 4 B x outputs written per particle) and the fraction of 8 TB/s they come to.

    python tools/particle_time.py --steps 20 [--emitters 256] [--particles 65536]
    python tools/particle_time.py --reference [--steps 3]    # the CPU baseline: the reference's own code, one thread, the same workload

--reference cuts the reference's particle VM out of its tree as tests/test_particle_oracle_vs_ref.py does (it needs that tree and no GPU).
No bar is fixed. Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run (tools/gpu_cases/particles.sh).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import particle_asm as A  # noqa: E402
from tests.particle_asm import CH, REG, LIT, SYS, GLOB, OUT  # noqa: E402

CHANNELS, OUTPUTS = 8, 12  # x y z, vx vy vz, age, size


def workload(particles):
    dt = SYS(A.TIME_DELTA)
    emit = [A.mul(REG(0), SYS(A.EMIT_INDEX), LIT(0.001)), A.sin(CH(0), REG(0)), A.cos(CH(2), REG(0)), A.mov(CH(1), SYS(A.ENTITY_Y)), A.mul(CH(3), CH(0), LIT(2.0)),
            A.mov(CH(4), LIT(5.0)), A.mul(CH(5), CH(2), LIT(2.0)), A.mov(CH(6), LIT(0.0)), A.mov(CH(7), LIT(1.0))]
    update = [
        A.madd(CH(4), dt, GLOB(0), CH(4)),                                                  # gravity
        A.mul(REG(0), dt, GLOB(1)), A.sub(REG(0), LIT(1.0), REG(0)),                          # drag factor
        A.mul(CH(3), CH(3), REG(0)), A.mul(CH(4), CH(4), REG(0)), A.mul(CH(5), CH(5), REG(0)),
        A.add(REG(1), CH(6), CH(0)), A.noise(REG(2), REG(1)), A.madd(CH(3), REG(2), dt, CH(3)),   # wobble
        A.madd(CH(0), CH(3), dt, CH(0)), A.madd(CH(1), CH(4), dt, CH(1)), A.madd(CH(2), CH(5), dt, CH(2)),
        A.add(CH(6), CH(6), dt),
        A.lt(REG(3), CH(1), LIT(0.0)), A.mul(REG(4), CH(4), LIT(-0.6)), A.blend(CH(4), CH(4), REG(4), REG(3)), A.max_(CH(1), CH(1), LIT(0.0)),   # bounce
        A.div(REG(5), CH(6), GLOB(2)), A.mix(CH(7), LIT(1.0), LIT(0.1), REG(5)), A.min_(CH(7), CH(7), LIT(1.0)),
        A.mul(REG(6), CH(3), CH(3)), A.madd(REG(6), CH(4), CH(4), REG(6)), A.madd(REG(6), CH(5), CH(5), REG(6)), A.sqrt(REG(6), REG(6)),
        A.mul(REG(6), REG(6), LIT(0.01)), A.add(CH(7), CH(7), REG(6)),
        A.gt(REG(7), CH(6), GLOB(2)), A.cmp(REG(7), [A.KILL]),
    ]
    assert len(update) + 2 == 30  # with the block's KILL and END
    output = [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1)), A.mov(OUT(2), CH(2)), A.mov(OUT(3), CH(7)), A.div(REG(0), CH(6), GLOB(2)),
              A.gradient(OUT(4), REG(0), [0.0, 0.3, 1.0], [1.0, 0.9, 0.2]), A.gradient(OUT(5), REG(0), [0.0, 0.5, 1.0], [0.8, 0.4, 0.1]), A.mix(OUT(6), LIT(0.2), LIT(0.0), REG(0)),
              A.sub(OUT(7), LIT(1.0), REG(0)), A.mov(OUT(8), CH(3)), A.mov(OUT(9), CH(4)), A.mov(OUT(10), CH(5)), A.mov(OUT(11), CH(6))]
    return A.Program(update, emit, output, channels=CHANNELS, registers=8, outputs=OUTPUTS, init_emit_count=particles)


GLOBALS = [-9.81, 0.2, 1.0e9]  # gravity, drag, lifetime (nobody dies inside the timed steps: the count stays what it is)


def reference(args):
    from tests import test_particle_oracle_vs_ref as R

    d = tempfile.mkdtemp(prefix="particle_time_ref_")
    exe = R.build_harness(d)
    p = workload(args.particles)
    job = os.path.join(d, "job.bin")
    open(job, "wb").write(R.job_bytes([[p]] * args.emitters, [1.0 / 60] * (1 + args.steps), GLOBALS, np.zeros((args.emitters, 3))))
    lines = subprocess.run([exe, job, os.path.join(d, "out.bin"), "time"], check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [[float(x) for x in l.split()] for l in lines if l.strip()][1:]  # the first step emits
    print(json.dumps({"what": "the reference's ParticleSystem::update + fillInstanceData, sliced, one thread", "emitters": args.emitters, "particles": int(rows[0][0]),
                      "steps": len(rows), "update_ms_median": float(np.median([r[1] for r in rows])), "fill_ms_median": float(np.median([r[2] for r in rows]))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--emitters", type=int, default=256)
    ap.add_argument("--particles", type=int, default=65536)
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    if args.reference:
        if args.steps == 20:
            args.steps = 3
        return reference(args)
    import torch

    from lumixengine_amd import api

    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB (torch opens the device before the library does)
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ps = api.ParticleSystems(ctx)
    p = workload(args.particles)
    for s in range(args.emitters):
        ps.addSystem(1, len(GLOBALS))
        ps.setGlobals(s, GLOBALS)
        p.set_on(ps, s, 0)
        ps.reserve(s, 0, args.particles)
    ps.setEntityPositions(np.zeros((args.emitters, 3)))
    ps.update(1.0 / 60)  # the first step emits
    ps.fill()
    total = int(ps.counts()["particles"].sum())
    assert total == args.emitters * args.particles, total

    def spans(cold):
        t = []
        for k in range(3 + args.steps):
            if cold:
                scrub.fill_(float(k))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ps.update(1.0 / 60)
            ps.fill()
            b.record()
            b.synchronize()
            if k >= 3:
                t.append(a.elapsed_time(b) * 1e3)
        return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}

    warm, cold = spans(False), spans(True)
    bytes_algo = total * 4 * (2 * CHANNELS + OUTPUTS)
    out = {"emitters": args.emitters, "particles": total, "steps": args.steps, "warm": warm, "behind_1GiB_scrub": cold, "algorithmic_bytes": bytes_algo,
           "fraction_of_8TBps_warm": bytes_algo / (warm["median_us"] * 1e-6) / 8e12, "particles_after": int(ps.counts()["particles"].sum())}
    ps.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
