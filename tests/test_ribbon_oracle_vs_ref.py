"""Pins tests/ribbon_oracle.py to the reference's own code (CPU; skipped where the reference tree is absent).

The method is that of tests/test_particle_oracle_vs_ref.py, whose shim and slices this file extends at test time: emitRibbonPoints,
applyTransform, updateRibbons, killRibbon and emitRibbons are cut out of renderer/particle_system.cpp next to what that file already cuts,
the shim's ParticleSystem gets Emitter::ribbons, last_emit_point (zeroed: deviation d) and the previous transform, and a driver of its own
runs the scripts of tests/ribbon_cases.py op by op. Nothing of the reference is committed.

After every op the oracle must equal the reference bit for bit: particles_count, every ribbon record, every live point of every channel.
The fill is pinned in two ways. Where the reference is self-consistent - one ribbon, or every ribbon but the last full - its own
fillInstanceData must give the oracle's packed bytes. For any lengths, the driver also runs the reference's output program over every
physical slot (particles_count set to ribbons x max_len for that call), and the oracle's packed rows must be exactly the gather of those
rows by points_offset."""
import os
import subprocess

import numpy as np
import pytest

from tests import ribbon_cases as C
from tests import test_particle_oracle_vs_ref as P
from tests.test_gpu_particles import assert_bits
from tests.test_im_oracle_vs_ref import FLAGS, REF

MAIN = r"""
int main(int argc, char** argv) {
	FILE* f = fopen(argv[1], "rb");
	FILE* o = fopen(argv[2], "wb");
	if (!f || !o) return 2;
	Heap heap;
	PageAllocator pages;
	const u32 n_systems = rd<u32>(f);
	std::vector<World> worlds(n_systems);
	std::vector<ParticleSystemResource> resources(n_systems);
	std::vector<ParticleSystem*> systems;
	for (u32 s = 0; s < n_systems; ++s) {
		worlds[s].pos.x = rd<double>(f); worlds[s].pos.y = rd<double>(f); worlds[s].pos.z = rd<double>(f);
		ParticleSystem* ps = new ParticleSystem(worlds[s], heap);
		ps->m_resource = &resources[s];
		ps->m_prev_frame_transform = Transform::IDENTITY;
		const u32 n_emitters = rd<u32>(f);
		resources[s].m_emitters.v.resize(n_emitters);
		for (u32 e = 0; e < n_emitters; ++e) {
			ParticleSystemResource::Emitter& r = resources[s].m_emitters.v[e];
			r.emit_offset = rd<u32>(f); r.output_offset = rd<u32>(f); r.channels_count = rd<u32>(f);
			r.update_registers_count = r.emit_registers_count = r.output_registers_count = rd<u32>(f);
			r.outputs_count = rd<u32>(f); r.emit_inputs_count = rd<u32>(f); r.init_emit_count = rd<u32>(f);
			r.max_ribbons = rd<u32>(f); r.max_ribbon_length = rd<u32>(f); r.init_ribbons_count = rd<u32>(f);
			r.emit_per_second = rd<float>(f); r.emit_move_distance = rd<float>(f);
			r.instructions.v.resize(rd<u32>(f));
			if (fread(r.instructions.v.data(), 1, r.instructions.v.size(), f) != r.instructions.v.size()) return 2;
		}
		ps->m_emitters.v.reserve(n_emitters);
		for (u32 e = 0; e < n_emitters; ++e) ps->m_emitters.v.emplace_back(*ps, resources[s].m_emitters.v[e]);
		systems.push_back(ps);
	}
	const u32 n_ops = rd<u32>(f);
	for (u32 k = 0; k < n_ops; ++k) {
		const u32 kind = rd<u32>(f);
		if (kind == 0) {
			const float dt = rd<float>(f);
			for (ParticleSystem* ps : systems) ps->update(dt, pages);
		} else if (kind == 1) {
			const u32 s = rd<u32>(f), e = rd<u32>(f), n = rd<u32>(f);
			worlds[s].pos = worlds[s].pos; // (emitRibbonPoints reads the entity's position itself)
			systems[s]->emitRibbons(e, n);
		} else if (kind == 2) {
			const u32 s = rd<u32>(f), e = rd<u32>(f), r = rd<u32>(f);
			systems[s]->killRibbon(e, r);
		} else {
			for (u32 s = 0; s < n_systems; ++s) {
				Transform tr = Transform::IDENTITY;
				tr.pos.x = rd<double>(f); tr.pos.y = rd<double>(f); tr.pos.z = rd<double>(f);
				worlds[s].pos = tr.pos; // the entity is where its transform is
				systems[s]->applyTransform(tr);
			}
		}
		for (ParticleSystem* ps : systems)
			for (ParticleSystem::Emitter& em : ps->m_emitters.v) {
				const ParticleSystemResource::Emitter& r = em.resource_emitter;
				const u32 n = em.particles_count, nr = (u32)em.ribbons.size();
				const u32 slots = r.max_ribbons ? r.max_ribbons * r.max_ribbon_length : n;
				fwrite(&n, 4, 1, o); fwrite(&em.emit_index, 4, 1, o); fwrite(&nr, 4, 1, o);
				for (const ParticleSystem::Ribbon& rb : em.ribbons.v) { fwrite(&rb.offset, 4, 1, o); fwrite(&rb.length, 4, 1, o); fwrite(&rb.emit_index, 4, 1, o); }
				std::vector<float> zeros(slots, 0.0f);
				for (u32 c = 0; c < r.channels_count; ++c) fwrite(em.channels[c].data ? em.channels[c].data : zeros.data(), 4, slots, o);
				std::vector<float> slice(em.getParticlesDataSizeBytes() / 4 + 4, 0.0f);
				em.fillInstanceData(slice.data(), pages);
				fwrite(slice.data(), 4, (size_t)n * r.outputs_count, o);
				if (r.max_ribbons) { // the output program over every physical slot of the live ribbons
					const u32 all = nr * r.max_ribbon_length;
					std::vector<float> phys((size_t)all * r.outputs_count + 16, 0.0f);
					em.particles_count = all;
					em.fillInstanceData(phys.data(), pages);
					em.particles_count = n;
					fwrite(phys.data(), 4, (size_t)all * r.outputs_count, o);
				}
			}
	}
	fclose(o);
	return 0;
}
"""


def harness():
    h = P.HARNESS

    def rep(a, b):
        nonlocal h
        assert h.count(a) == 1, a
        h = h.replace(a, b)

    rep("\tu32 byte_size() const { return (u32)(v.size() * sizeof(T)); }\n};",
        "\tu32 byte_size() const { return (u32)(v.size() * sizeof(T)); }\n\tvoid erase(u32 i) { v.erase(v.begin() + i); }\n\tvoid resize(u32 n) { v.resize(n); }\n\tvoid reserve(u32 n) { v.reserve(n); }\n};")
    rep("\t\tfloat emit_per_second;\n\t};", "\t\tfloat emit_per_second;\n\t\tfloat emit_move_distance = -1;\n\t};")
    rep("\tstruct Emitter {\n\t\tEmitter(ParticleSystem& system,", "\tstruct Ribbon { u32 offset, length, emit_index; };\n\tstruct Emitter {\n\t\tEmitter(ParticleSystem& system,")
    rep("\t\tfloat emit_timer = 0;\n\t};", "\t\tfloat emit_timer = 0;\n\t\tArr<Ribbon> ribbons;\n\t\tDVec3 last_emit_point = DVec3(0, 0, 0);\n\t};")
    rep("\tvoid updateRibbons(float, u32, PageAllocator&) {}\n\tvoid emitRibbons(u32, u32) {}\n",
        "\tvoid updateRibbons(float dt, u32 emitter_idx, PageAllocator& page_allocator);\n\tvoid emitRibbons(u32 emitter_idx, u32 num_ribbons);\n"
        "\tvoid emitRibbonPoints(u32 emitter_idx, u32 ribbon_idx, Span<const float> emit_data, u32 count, float time_step);\n"
        "\tvoid killRibbon(u32 emitter_idx, u32 ribbon_index);\n\tvoid applyTransform(const Transform& new_tr);\n\tTransform m_prev_frame_transform;\n")
    return h[:h.index("int main(int argc, char** argv) {")] + MAIN


def slice_ribbons(out_dir):
    P.slice_reference(out_dir)
    ps = open(os.path.join(REF, "src", "renderer", "particle_system.cpp")).read()
    parts = [P._between(ps, "void ParticleSystem::emitRibbonPoints", "void ParticleSystem::emit(u32 emitter_idx")[0],
             P._between(ps, "void ParticleSystem::applyTransform", "void ParticleSystem::update(float dt, u32 emitter_idx")[0],
             P._between(ps, "void ParticleSystem::killRibbon", "bool ParticleSystem::update(float dt, PageAllocator")[0]]
    assert "ribbon.offset + ribbon.length - 1" in parts[0] and "squaredLength(new_tr.pos - emitter.last_emit_point)" in parts[1] and "memmove" in parts[2]
    with open(os.path.join(out_dir, "particle_slices.inc"), "a") as f:
        f.write("\n" + "\n".join(parts))


def build_harness(d):
    """the sliced reference with its ribbon path behind the shim, compiled in directory `d`: the program's path"""
    slice_ribbons(str(d))
    open(os.path.join(str(d), "harness.cpp"), "w").write(harness())
    inc = ["-I" + str(d), "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "external")]
    objs = []
    for path in (os.path.join(str(d), "harness.cpp"), os.path.join(REF, "src", "core", "math.cpp")):
        obj = os.path.join(str(d), os.path.basename(path) + ".o")
        r = subprocess.run(["g++"] + FLAGS + ["-msse4.1"] + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-6000:]
        objs.append(obj)
    exe = os.path.join(str(d), "ribbons_ref")
    r = subprocess.run(["g++"] + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def job_bytes(case):
    systems, options, _, ops = C.CASES[case]
    job = bytearray(np.uint32(len(systems)).tobytes())
    for si, progs in enumerate(systems):
        job += np.zeros(3, np.float64).tobytes() + np.uint32(len(progs)).tobytes()
        for ei, p in enumerate(progs):
            o = options[si][ei]
            job += np.array([p.emit_offset, p.output_offset, p.channels, p.registers, p.outputs, p.emit_inputs, p.init_emit_count, o.max_ribbons, o.max_ribbon_length,
                             o.init_ribbons_count], np.uint32).tobytes()
            job += np.float32(p.emit_per_second).tobytes() + np.float32(o.emit_move_distance).tobytes() + np.uint32(len(p.bytes)).tobytes() + p.bytes
    job += np.uint32(len(ops)).tobytes()
    for op in ops:
        if op[0] == "step": job += np.uint32(0).tobytes() + np.float32(op[1]).tobytes()
        elif op[0] == "emit_ribbons": job += np.array([1, *op[1:]], np.uint32).tobytes()
        elif op[0] == "kill": job += np.array([2, *op[1:]], np.uint32).tobytes()
        else: job += np.uint32(3).tobytes() + np.asarray(op[1], np.float64).tobytes()
    return bytes(job)


def run_reference(exe, d, case):
    """[per op: [per emitter: (count, emit_index, records, live points [channels, n], the reference's own slice rows, the rows of every physical slot or None)]]"""
    systems, options, _, ops = C.CASES[case]
    jp, op_ = os.path.join(str(d), case + ".job"), os.path.join(str(d), case + ".out")
    open(jp, "wb").write(job_bytes(case))
    subprocess.run([exe, jp, op_], check=True, timeout=300)
    b, at, trace = open(op_, "rb").read(), 0, []
    for _ in ops:
        state = []
        for si, progs in enumerate(systems):
            for ei, p in enumerate(progs):
                o = options[si][ei]
                n, eidx, nr = (int(x) for x in np.frombuffer(b, np.uint32, 3, at))
                at += 12
                rec = np.frombuffer(b, np.uint32, 3 * nr, at).reshape(nr, 3)
                at += 12 * nr
                slots = o.max_ribbons * o.max_ribbon_length if o.max_ribbons else n
                ch = np.frombuffer(b, np.float32, p.channels * slots, at).reshape(p.channels, slots)
                at += 4 * p.channels * slots
                rows = np.frombuffer(b, np.float32, n * p.outputs, at)
                at += 4 * n * p.outputs
                phys = None
                if o.max_ribbons:
                    L = o.max_ribbon_length
                    phys = np.frombuffer(b, np.float32, nr * L * p.outputs, at).reshape(nr * L, p.outputs)
                    at += 4 * nr * L * p.outputs
                    cols = np.concatenate([np.arange(r * L, r * L + int(rec[r, 1])) for r in range(nr)] + [np.zeros(0, np.int64)]).astype(np.int64)
                    ch = ch[:, cols]
                state.append((n, eidx, [tuple(int(x) for x in r) for r in rec], ch, rows, phys))
        trace.append(state)
    assert at == len(b)
    return trace


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    if not os.path.isdir(os.path.join(REF, "src")):
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("ribbons_ref")
    return build_harness(d), d


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_oracle_equals_the_reference(ref_exe, case):
    exe, d = ref_exe
    systems, options, _, ops = C.CASES[case]
    want, got = run_reference(exe, d, case), C.run_oracle(case)
    consistent = 0
    for k, (ws, gs) in enumerate(zip(want, got)):
        g = 0
        for si, progs in enumerate(systems):
            for ei, p in enumerate(progs):
                (n, eidx, rec, ch, rows, phys), (gn, geidx, grec, gch, grows) = ws[g], gs[g]
                what = f"{case}, op {k} {ops[k][0]}, system {si} emitter {ei}"
                assert (n, eidx) == (gn, geidx), what
                g += 1
                if phys is None:
                    assert_bits(gch, ch, f"{what}: channels, oracle (got) against reference (want)")
                    assert_bits(grows, rows, f"{what}: slice")
                    continue
                assert [r[:3] for r in grec] == rec, what
                assert_bits(gch, ch, f"{what}: live points, oracle (got) against reference (want)")
                L, lens = options[si][ei].max_ribbon_length, [r[1] for r in rec]
                if len(lens) <= 1 or all(x == L for x in lens[:-1]):  # the reference's fill is self-consistent: its bytes
                    assert_bits(grows, rows, f"{what}: slice against the reference's own")
                    consistent += len(lens) > 0
                gather = np.concatenate([phys[r * L:r * L + lens[r]] for r in range(len(lens))] + [np.zeros((0, p.outputs), np.float32)])
                assert_bits(grows, gather.reshape(-1), f"{what}: packed rows against the gather of the physical rows")
                assert [r[3] for r in grec] == [sum(lens[:r]) * p.outputs * 4 for r in range(len(lens))], what
    if case in ("ring", "ring_two", "order"):
        assert consistent > 0
