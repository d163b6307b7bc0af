#!/usr/bin/env python
"""Times one step plus fill of particle systems whose programs read their entity (MESH and SPLINE). The workload:
--systems systems of one emitter with --particles particles each, all on ONE skinned model (--bones bones, --verts vertices, uploaded
once) with a skin instance and a spline each. The emit program draws a vertex and places the particle on it; an update block re-reads
the vertex every step (three MESH per particle and step); the output program moves the particle's colour along the spline (one SPLINE).
The same run with every MESH / SPLINE replaced by a MOV of the same operands gives the cost of the two instructions as a difference.
Median of --steps spans between stream events, warm (back to back) and behind a 1 GiB scrub of the caches; one JSON line.

    python tools/particle_source_time.py --steps 20 [--systems 256] [--particles 4096] [--bones 64] [--verts 10000]

No bar is fixed: no number for the two instructions existed before this tool.
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

CHANNELS, OUTPUTS = 5, 5  # the vertex index, x y z, age


def workload(particles, sources):
    """sources=False: the same programs with MOV in the place of every MESH / SPLINE"""
    mesh = A.mesh if sources else (lambda dst, index, sub: A.mov(dst, index))
    spline = A.spline if sources else (lambda dst, src, sub: A.mov(dst, src))
    place = [mesh(CH(1), CH(0), 0), mesh(CH(2), CH(0), 1), mesh(CH(3), CH(0), 2)]
    emit = [A.mov(CH(0), LIT(-1.0) if sources else SYS(A.EMIT_INDEX))] + place + [A.mov(CH(4), LIT(0.0))]
    update = [A.add(CH(4), CH(4), SYS(A.TIME_DELTA)), A.sub(REG(0), LIT(0.0), LIT(1.0)), A.cmp(REG(0), place)]  # the block's condition: the sign bit, always
    output = [A.mov(OUT(0), CH(1)), A.mov(OUT(1), CH(2)), A.mov(OUT(2), CH(3)), A.mov(OUT(3), CH(4)), A.mul(REG(0), CH(4), LIT(0.25)), spline(OUT(4), REG(0), 1)]
    return A.Program(update, emit, output, channels=CHANNELS, registers=1, outputs=OUTPUTS, init_emit_count=particles)


def measure(args, torch, api, scenes, scrub, sources):
    ctx = api.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    sk = api.Skinning(ctx)
    sk.setMode(True)
    skel = scenes.skeleton(args.bones, seed=4)
    verts, skin = scenes.skinned_mesh(args.verts, args.bones, seed=6)
    model, smesh = sk.addModel(skel["parents"], skel["bind"], skel["first_nonroot"]), sk.addMesh(verts, skin)
    sk.setInstances([model] * args.systems, [smesh] * args.systems)
    pos, rot = scenes.relative_poses(args.systems, args.bones, seed=5)
    sk.uploadPoses(pos.reshape(-1, 3), rot.reshape(-1, 4))
    sk.run()
    ps = api.ParticleSystems(ctx)
    p = workload(args.particles, sources)
    mesh = ps.addMesh(verts, skin)  # one upload for every system
    pts = np.random.default_rng(8).uniform(-1, 1, size=(8, 3)).astype(np.float32)
    for s in range(args.systems):
        ps.addSystem(1)
        ps.setMeshSource(s, mesh, s, api.PARTICLE_MESH_HAS_BONES)
        ps.setSpline(s, pts)
        p.set_on(ps, s, 0)
        ps.reserve(s, 0, args.particles)
    dt = 1.0 / 60.0
    ps.update(dt)
    ps.fill()
    total = int(ps.counts()["particles"].sum())
    assert total == args.systems * args.particles, total

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

    out = {"warm": spans(False), "behind_1GiB_scrub": spans(True), "live_particles": total}
    ps.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--verts", type=int, default=10000)
    args = ap.parse_args()
    import torch

    from lumixengine_amd import api, scenes

    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda")  # 1 GiB (torch opens the device before the library does)
    with_sources = measure(args, torch, api, scenes, scrub, True)
    with_mov = measure(args, torch, api, scenes, scrub, False)
    n = with_sources["live_particles"]
    extra = with_sources["warm"]["median_us"] - with_mov["warm"]["median_us"]
    out = {"systems": args.systems, "particles_per_system": args.particles, "bones": args.bones, "verts": args.verts, "steps": args.steps,
           "mesh_per_particle_step": 3, "spline_per_particle_fill": 1, "with_mesh_and_spline": with_sources, "with_mov_instead": with_mov,
           "difference_warm_us": extra, "difference_ns_per_particle": extra * 1e3 / n,
           "per_mesh_bytes_read": 12 + 24 + 4 * 16}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
