#!/usr/bin/env python
"""Times one step plus fill of ribbon emitters on the device. The workload is trails: --systems systems x 1 emitter x --ribbons ribbons x
--points points (every ring full before the timed steps), one point a step into every ribbon, a short update program (an age, a fade, a
drift) and a 6-float output program. Median of --steps spans between stream events, warm (back to back) and behind a 1 GiB scrub of the
caches; one JSON line with the algorithmic bytes per step (4 B x channels read and written + 4 B x outputs written per live point) and
the fraction of 8 TB/s they come to.

    python tools/ribbon_time.py --steps 20 [--systems 1024] [--ribbons 16] [--points 64]

No bar is fixed. There is no CPU baseline yet: it needs the reference's ribbon path cut out of its tree behind a shim, as
tools/particle_time.py --reference does for the sprite path.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import particle_asm as A  # noqa: E402
from tests.particle_asm import CH, REG, LIT, SYS, OUT  # noqa: E402

CHANNELS, OUTPUTS = 6, 6  # x y z, age, alpha, width
RATE = 60.0


def workload(points):
    dt = SYS(A.TIME_DELTA)
    emit = [A.mov(CH(0), SYS(A.ENTITY_X)), A.mov(CH(1), SYS(A.ENTITY_Y)), A.mov(CH(2), SYS(A.ENTITY_Z)), A.mov(CH(3), LIT(0.0)), A.mov(CH(4), LIT(1.0)),
            A.madd(CH(5), SYS(A.RIBBON_INDEX), LIT(0.01), LIT(0.1))]
    update = [A.add(CH(3), CH(3), dt), A.mul(REG(0), CH(3), LIT(0.5)), A.sub(CH(4), LIT(1.0), REG(0)), A.max_(CH(4), CH(4), LIT(0.0)), A.madd(CH(1), dt, LIT(0.2), CH(1)),
              A.madd(CH(5), dt, LIT(0.05), CH(5))]
    output = [A.mov(OUT(0), CH(0)), A.mov(OUT(1), CH(1)), A.mov(OUT(2), CH(2)), A.mov(OUT(3), CH(4)), A.mov(OUT(4), CH(5)), A.mov(OUT(5), CH(3))]
    return A.Program(update, emit, output, channels=CHANNELS, registers=1, outputs=OUTPUTS, init_emit_count=points, emit_per_second=RATE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--systems", type=int, default=1024)
    ap.add_argument("--ribbons", type=int, default=16)
    ap.add_argument("--points", type=int, default=64)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api

    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB (torch opens the device before the library does)
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ps = api.ParticleSystems(ctx)
    p = workload(args.points)
    for s in range(args.systems):
        ps.addSystem(1)
        p.set_on(ps, s, 0)
        ps.setEmitterOptions(s, 0, args.ribbons, args.points, args.ribbons)
    ps.setEntityPositions(np.zeros((args.systems, 3)))
    dt = 1.0 / RATE + 1.0e-4  # one point a step into every ribbon
    ps.update(dt)  # the first step makes the ribbons, every ring full
    ps.fill()
    total = int(ps.counts()["particles"].sum())
    assert total == args.systems * args.ribbons * ((args.points + 3) & ~3), total

    def spans(cold):
        t = []
        for k in range(3 + args.steps):
            if cold:
                scrub.fill_(float(k))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ps.update(dt)
            ps.fill()
            b.record()
            b.synchronize()
            if k >= 3:
                t.append(a.elapsed_time(b) * 1e3)
        return {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}

    warm, cold = spans(False), spans(True)
    bytes_algo = total * 4 * (2 * CHANNELS + OUTPUTS)
    out = {"systems": args.systems, "ribbons": args.ribbons, "points": args.points, "live_points": total, "steps": args.steps, "warm": warm, "behind_1GiB_scrub": cold,
           "algorithmic_bytes_per_step": bytes_algo, "fraction_of_8TBps_warm": bytes_algo / (warm["median_us"] * 1e-6) / 8e12,
           "live_points_after": int(ps.counts()["particles"].sum())}
    ps.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
