"""Pins tests/particle_oracle.py to the reference's own code (CPU; skipped where the reference tree is absent).

At test time hash / gnoise, ensureCapacity, emit, getStream / ProcessHelper, run, ChunkProcessorContext, processChunk, the per-emitter update,
the system's update, getParticlesDataSizeBytes and fillInstanceData are cut out of renderer/particle_system.cpp, and the intrinsic branch of
core/simd.h (the engine's shipping form, DESIGN §4.15 deviation 1) out of that header, into a temporary directory and compiled with
-msse2 -msse4.1 -mfpmath=sse -ffp-contract=off behind the shim below, with core/math.cpp compiled in place (lerp, randFloat). Nothing of the
reference is committed: the shim only declares the containers the slices touch (streams, pages, a stack array, the resource's emitter
record, the world's position) with the members they call. The MESH and SPLINE cases are cut away with the text (they need the renderer).

The programs are those of tests/test_gpu_particles.py: its test functions are run with the device replaced by the compiled reference, so
the oracle must equal the reference bit for bit - every count, every channel value and slice row in [0, count), after every step - on
what the device is compared with. Left out: RAND (deviation 5; its formula is pinned with RandomGenerator::randFloat fed the same u32)
and the capacity cases (deviation 8: the reference grows)."""
import os
import subprocess

import numpy as np
import pytest

from tests import particle_oracle as O
from tests import test_gpu_particles as S
from tests.test_im_oracle_vs_ref import FLAGS, REF

HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>
#include <xmmintrin.h>
#include <smmintrin.h>
#include "core/allocator.h"
#include "core/math.h"
#include "core/metaprogramming.h"
#include "core/span.h"
#include "engine/lumix.h"

#define PROFILE_FUNCTION()
#define PROFILE_BLOCK(x)

namespace Lumix {
#include "simd_intrinsic.inc"

namespace profiler { inline void pushInt(const char*, int) {} }
namespace jobs {
struct Mutex {};
inline void enter(Mutex*) {}
inline void exit(Mutex*) {}
template <typename F> void runOnWorkers(F& f) { f(); } // one worker: chunks in ascending order
}
template <typename... A> void logError(A...) {}

struct Heap final : IAllocator {
	void* allocate(size_t size, size_t align) override { return calloc(1, (size + 63) / 16 * 16 + 64); }
	void deallocate(void* p) override { free(p); }
	void* reallocate(void* p, size_t n, size_t old, size_t align) override {
		void* q = allocate(n, align);
		if (p) { memcpy(q, p, old < n ? old : n); free(p); }
		return q;
	}
};
struct AtomicI32 {
	i32 value;
	AtomicI32(i32 v = 0) : value(v) {}
	i32 add(i32 v) { const i32 o = value; value += v; return o; } // returns the initial value (core/atomic.h)
};
struct PageAllocator {
	enum { PAGE_SIZE = 4096 };
	void* allocate() { return calloc(1, PAGE_SIZE); }
	void deallocate(void* p) { free(p); }
};
template <typename T> struct Arr {
	std::vector<T> v;
	int size() const { return (int)v.size(); }
	T* begin() { return v.data(); }
	T* end() { return v.data() + v.size(); }
	const T* begin() const { return v.data(); }
	const T* end() const { return v.data() + v.size(); }
	T& operator[](u32 i) { return v[i]; }
	const T& operator[](u32 i) const { return v[i]; }
	u32 byte_size() const { return (u32)(v.size() * sizeof(T)); }
};
template <typename T, u32 N> struct StackArray : Arr<T> {
	StackArray(IAllocator&) {}
	void resize(u32 n) { this->v.resize(n); }
	bool empty() const { return this->v.empty(); }
	void push(const T& x) { this->v.push_back(x); }
	void pop() { this->v.pop_back(); }
	T& last() { return this->v.back(); }
};
struct Bytes {
	std::vector<u8> v;
	const u8* data() const { return v.data(); }
	u64 size() const { return v.size(); }
};
struct InputMemoryStream {
	const u8* m_data; u64 m_size, m_pos = 0;
	InputMemoryStream(const void* d, u64 s) : m_data((const u8*)d), m_size(s) {}
	InputMemoryStream(const Bytes& b) : m_data(b.data()), m_size(b.size()) {}
	void set(const void* d, u64 s) { m_data = (const u8*)d; m_size = s; m_pos = 0; }
	bool read(void* out, u64 n) { if (m_pos + n > m_size) { fprintf(stderr, "read past the stream\n"); ::exit(3); } memcpy(out, m_data + m_pos, n); m_pos += n; return true; }
	template <typename T> T read() { T v; read(&v, sizeof(T)); return v; }
	template <typename T> void read(T& v) { read(&v, sizeof(T)); }
	void skip(u64 n) { m_pos += n; }
	const void* getData() const { return m_data; }
	u64 getPosition() const { return m_pos; }
	void setPosition(u64 p) { m_pos = p; }
};
struct OutputPagedStream {
	std::vector<u8> v;
	OutputPagedStream(PageAllocator&) {}
	void write(const void* p, u64 n) { v.insert(v.end(), (const u8*)p, (const u8*)p + n); }
	template <typename T> void write(const T& x) { write(&x, sizeof(T)); }
};
struct InputPagedStream {
	const std::vector<u8>& v; u64 pos = 0;
	InputPagedStream(const OutputPagedStream& o) : v(o.v) {}
	bool isEnd() const { return pos >= v.size(); }
	void read(void* out, u64 n) { memcpy(out, v.data() + pos, n); pos += n; }
	template <typename T> T read() { T x; read(&x, sizeof(T)); return x; }
};
struct World {
	DVec3 pos;
	DVec3 getPosition(EntityRef) const { return pos; }
};

struct ParticleSystemResource {
	struct DataStream {
		enum Type : u8 { NONE, CHANNEL, SYSTEM_VALUE, OUT, REGISTER, LITERAL, GLOBAL, ERROR };
		Type type = NONE;
		u8 index;
		float value;
	};
	enum class InstructionType : u8 { END, ADD, COS, SIN, NOISE, SUB, EMIT, MUL, MULTIPLY_ADD, LT, MOV, RAND, KILL, SQRT, GT, MIX, GRADIENT, DIV, SPLINE, MESH, MOD, OR, AND,
		NOT, BLEND, MAX, MIN, CMP, CMP_ELSE };
	struct Emitter {
		Bytes instructions;
		u32 emit_offset, output_offset, channels_count, update_registers_count, emit_registers_count, output_registers_count, outputs_count, init_emit_count,
			emit_inputs_count, max_ribbons = 0, max_ribbon_length = 0, init_ribbons_count = 0;
		float emit_per_second;
	};
	Arr<Emitter> m_emitters;
	Arr<Emitter>& getEmitters() { return m_emitters; }
	bool isReady() const { return true; }
};
using DataStream = ParticleSystemResource::DataStream;
using InstructionType = ParticleSystemResource::InstructionType;
enum class ParticleSystemValues : u8 { TIME_DELTA = 0, TOTAL_TIME = 1, EMIT_INDEX = 2, RIBBON_INDEX = 3, ENTITY_POSITION_X = 4, ENTITY_POSITION_Y = 5, ENTITY_POSITION_Z = 6, COUNT };
struct EmSpan {
	ParticleSystemResource::Emitter* p = nullptr;
	ParticleSystemResource::Emitter& operator[](u32 i) const { return p[i]; }
	void operator=(Arr<ParticleSystemResource::Emitter>& a) { p = a.begin(); }
};

struct ParticleSystem {
	struct Channel { float* data = nullptr; u32 name = 0; };
	struct Stats { AtomicI32 emitted = 0, killed = 0, processed = 0; };
	struct Emitter {
		Emitter(ParticleSystem& system, ParticleSystemResource::Emitter& resource_emitter) : system(system), resource_emitter(resource_emitter) {}
		u32 getParticlesDataSizeBytes() const;
		void fillInstanceData(float* data, PageAllocator& page_allocator) const;
		ParticleSystem& system;
		ParticleSystemResource::Emitter& resource_emitter;
		Channel channels[16];
		u32 particles_count = 0, capacity = 0, emit_index = 0;
		float emit_timer = 0;
	};
	enum class RunResult { SURVIVED, KILLED };
	struct RunningContext {
		bool is_ribbon = false;
		const Channel* channels = nullptr;
		const float* system_values = nullptr;
		const float* globals = nullptr;
		float* registers[16] = {};
		float* output_memory = nullptr;
		InputMemoryStream instructions = InputMemoryStream(nullptr, 0);
		u32 ribbon_index = 0, particle_idx = 0, register_access_idx = 0;
		World* world = nullptr;
		EntityPtr entity;
		EmSpan emitters;
		OutputPagedStream* emit_stream = nullptr;
		jobs::Mutex* emit_mutex = nullptr;
	};
	struct ChunkProcessorContext;
	ParticleSystem(World& world, IAllocator& allocator) : m_allocator(allocator), m_world(world) { m_entity.index = 0; }
	static RunResult run(RunningContext& ctx, IAllocator& tmp_allocator);
	void processChunk(ChunkProcessorContext& ctx);
	void ensureCapacity(Emitter& emitter, u32 num_new_particles);
	void emit(u32 emitter_idx, Span<const float> emit_data, u32 count, float time_step);
	void update(float dt, u32 emitter_idx, PageAllocator& page_allocator);
	bool update(float dt, PageAllocator& page_allocator);
	void updateRibbons(float, u32, PageAllocator&) {}
	void emitRibbons(u32, u32) {}
	IAllocator& m_allocator;
	World& m_world;
	EntityPtr m_entity;
	Arr<Emitter> m_emitters;
	Arr<float> m_globals;
	ParticleSystemResource* m_resource = nullptr;
	bool m_autodestroy = false;
	float m_total_time = 0;
	float m_system_values[16] = {};
	Stats m_last_update_stats;
};

#include "particle_slices.inc"
} // namespace Lumix

using namespace Lumix;
namespace Lumix { namespace os { struct Timer { static u64 getRawTimestamp(); }; } } // core/os.h: core/math.cpp seeds its thread-local generator with it
u64 Lumix::os::Timer::getRawTimestamp() { return 1; }
template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) exit(2); return v; }

int main(int argc, char** argv) {
	if (argc == 6 && !strcmp(argv[1], "rand")) { // RandomGenerator::randFloat(from, to) on a generator in the given state
		RandomGenerator g((u32)strtoul(argv[2], 0, 10), (u32)strtoul(argv[3], 0, 10));
		const float v = g.randFloat((float)atof(argv[4]), (float)atof(argv[5]));
		u32 b; memcpy(&b, &v, 4);
		printf("%u\n", b);
		return 0;
	}
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
		ps->m_globals.v.resize(rd<u32>(f));
		for (float& g : ps->m_globals.v) g = rd<float>(f);
		const u32 n_emitters = rd<u32>(f);
		resources[s].m_emitters.v.resize(n_emitters);
		for (u32 e = 0; e < n_emitters; ++e) {
			ParticleSystemResource::Emitter& r = resources[s].m_emitters.v[e];
			r.emit_offset = rd<u32>(f); r.output_offset = rd<u32>(f); r.channels_count = rd<u32>(f);
			r.update_registers_count = r.emit_registers_count = r.output_registers_count = rd<u32>(f); // overrideData sets all three to registers_count
			r.outputs_count = rd<u32>(f); r.emit_inputs_count = rd<u32>(f); r.init_emit_count = rd<u32>(f);
			r.emit_per_second = rd<float>(f);
			r.instructions.v.resize(rd<u32>(f));
			if (fread(r.instructions.v.data(), 1, r.instructions.v.size(), f) != r.instructions.v.size()) return 2;
		}
		ps->m_emitters.v.reserve(n_emitters);
		for (u32 e = 0; e < n_emitters; ++e) ps->m_emitters.v.emplace_back(*ps, resources[s].m_emitters.v[e]);
		systems.push_back(ps);
	}
	const u32 n_steps = rd<u32>(f);
	if (argc == 4 && !strcmp(argv[3], "time")) { // tools/particle_time.py --reference: update + fill of every system per step, one thread, milliseconds
		for (u32 k = 0; k < n_steps; ++k) {
			const float dt = rd<float>(f);
			std::vector<float> slice;
			const auto t0 = std::chrono::steady_clock::now();
			for (ParticleSystem* ps : systems) ps->update(dt, pages);
			const auto t1 = std::chrono::steady_clock::now();
			u64 particles = 0;
			for (ParticleSystem* ps : systems)
				for (const ParticleSystem::Emitter& em : ps->m_emitters) {
					slice.resize(em.getParticlesDataSizeBytes() / 4 + 4);
					em.fillInstanceData(slice.data(), pages);
					particles += em.particles_count;
				}
			const auto t2 = std::chrono::steady_clock::now();
			printf("%llu %.3f %.3f\n", (unsigned long long)particles, std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
		}
		return 0;
	}
	for (u32 k = 0; k < n_steps; ++k) {
		const float dt = rd<float>(f);
		for (ParticleSystem* ps : systems) ps->update(dt, pages);
		for (ParticleSystem* ps : systems)
			for (const ParticleSystem::Emitter& em : ps->m_emitters) {
				const u32 n = em.particles_count, nc = em.resource_emitter.channels_count, no = em.resource_emitter.outputs_count;
				fwrite(&n, 4, 1, o);
				fwrite(&em.emit_index, 4, 1, o);
				for (u32 c = 0; c < nc; ++c) fwrite(em.channels[c].data, 4, n, o);
				const u32 bytes = em.getParticlesDataSizeBytes();
				std::vector<float> slice(bytes / 4 + 4, 0.0f);
				em.fillInstanceData(slice.data(), pages);
				fwrite(slice.data(), 4, (size_t)n * no, o);
			}
	}
	fclose(o);
	return 0;
}
"""


def _between(text, start, end, after=0):
    a = text.index(start, after)
    return text[a:text.index(end, a)], a


def slice_reference(out_dir):
    src = os.path.join(REF, "src")
    ps = open(os.path.join(src, "renderer", "particle_system.cpp")).read()
    parts = []
    parts.append(_between(ps, "namespace {\n\tfloat hash(u32 n)", "void ParticleSystem::emitRibbonPoints")[0])  # hash, gnoise, ensureCapacity
    parts.append(_between(ps, "void ParticleSystem::emit(u32 emitter_idx", "void ParticleSystem::serialize")[0])
    vm, _ = _between(ps, "static float4* getStream(", "void ParticleSystem::applyTransform")
    mesh, _ = _between(vm, "\t\t\tcase InstructionType::MESH: {", "\t\t\tcase InstructionType::MUL: {")
    vm = vm.replace(mesh, "")  # run's MESH and SPLINE cases: they need the renderer and the spline module
    chunk_at = vm.index("void ParticleSystem::processChunk")
    spline, _ = _between(vm, "\t\t\tcase InstructionType::SPLINE: {", "\t\t\tcase InstructionType::GRADIENT: {", chunk_at)
    vm = vm.replace(spline, "")
    assert "f4MoveMask" in vm and "register_access_idx = particle_index" in vm and "ctx.emit_stream->write(emitter_idx)" in vm
    parts.append(vm)
    parts.append(_between(ps, "void ParticleSystem::update(float dt, u32 emitter_idx", "void ParticleSystem::killRibbon")[0])
    tail, _ = _between(ps, "bool ParticleSystem::update(float dt, PageAllocator", "} // namespace Lumix")
    assert "fillInstanceData" in tail and "m_total_time += dt" in tail
    parts.append(tail)
    open(os.path.join(out_dir, "particle_slices.inc"), "w").write("\n".join(parts))
    simd = open(os.path.join(src, "core", "simd.h")).read()
    # the intrinsic branch (`#if defined _WIN32 && !defined __clang__` ... `#else`) up to its operator overloads: g++'s __m128 has its own
    branch, _ = _between(simd, "\tusing float4 = __m128;", "\tLUMIX_FORCE_INLINE float4 operator +(float4 a, float4 b)")
    assert "_mm_movemask_ps" in branch and "_mm_blendv_ps" in branch and "_mm_min_ps" in branch
    open(os.path.join(out_dir, "simd_intrinsic.inc"), "w").write(branch)


@pytest.fixture(scope="module")
def ref_exe(tmp_path_factory):
    if not os.path.isdir(os.path.join(REF, "src")):
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("particles_ref")
    exe = build_harness(d)
    return exe, d


def build_harness(d):
    """the sliced reference behind the shim, compiled in directory `d`: the program's path"""
    slice_reference(str(d))
    open(os.path.join(str(d), "harness.cpp"), "w").write(HARNESS)
    inc = ["-I" + str(d), "-I" + os.path.join(REF, "src"), "-I" + os.path.join(REF, "external")]
    objs = []
    for path in (os.path.join(str(d), "harness.cpp"), os.path.join(REF, "src", "core", "math.cpp")):
        obj = os.path.join(str(d), os.path.basename(path) + ".o")
        r = subprocess.run(["g++"] + FLAGS + ["-msse4.1"] + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-6000:]
        objs.append(obj)
    exe = os.path.join(str(d), "particles_ref")
    r = subprocess.run(["g++"] + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def job_bytes(systems, dts, globals_=None, positions=None):
    job = bytearray(np.uint32(len(systems)).tobytes())
    for si, progs in enumerate(systems):
        job += np.asarray(positions[si] if positions is not None else (0.0, 0.0, 0.0), np.float64).tobytes()
        g = np.asarray(globals_ if globals_ is not None else [], np.float32)
        job += np.uint32(len(g)).tobytes() + g.tobytes() + np.uint32(len(progs)).tobytes()
        for p in progs:
            job += np.array([p.emit_offset, p.output_offset, p.channels, p.registers, p.outputs, p.emit_inputs, p.init_emit_count], np.uint32).tobytes()
            job += np.float32(p.emit_per_second).tobytes() + np.uint32(len(p.bytes)).tobytes() + p.bytes
    job += np.uint32(len(dts)).tobytes() + np.asarray(dts, np.float32).tobytes()
    return bytes(job)


class RefPair:
    """tests/test_gpu_particles.Pair with the compiled reference in the device's place: the steps are recorded with the oracle's state after
    each, and compared when the pair is closed."""
    exe = None
    runs = 0

    def __init__(self, ctx, systems, capacities, seed=0, globals_=None, positions=None):
        ng = len(globals_) if globals_ is not None else 0
        self.world = O.make_world(systems, capacities, seed, ng, positions)
        self.systems, self.globals, self.positions = systems, globals_, positions
        for sy in self.world.systems:
            if ng:
                sy.globals[:] = globals_
        self.dts, self.states = [], []

    def step(self, dt, check=True):
        self.dts.append(dt)
        self.world.step(dt)
        fills = self.world.fill()
        state, g = [], 0
        for sy in self.world.systems:
            for em in sy.emitters:
                assert not em.overflow, "the reference has no capacity: a case for the device alone"
                state.append((em.count, em.emit_index, em.ch[:, :em.count].copy(), fills[g][0][:em.count * em.p.outputs].copy()))
                g += 1
        self.states.append(state)

    def close(self):
        exe, d = RefPair.exe
        job = job_bytes(self.systems, self.dts, self.globals, self.positions)
        RefPair.runs += 1
        jp, op = d / f"job{RefPair.runs}.bin", d / f"out{RefPair.runs}.bin"
        jp.write_bytes(bytes(job))
        subprocess.run([exe, str(jp), str(op)], check=True, timeout=300)
        b, at = op.read_bytes(), 0
        for k, state in enumerate(self.states):
            g = 0
            for si, progs in enumerate(self.systems):
                for ei, p in enumerate(progs):
                    n, eidx = (int(x) for x in np.frombuffer(b, np.uint32, 2, at))
                    at += 8
                    want_n, want_eidx, want_ch, want_rows = state[g]
                    assert (n, eidx) == (want_n, want_eidx), f"step {k} system {si} emitter {ei}: reference count / emit_index {n} / {eidx}, oracle {want_n} / {want_eidx}"
                    ch = np.frombuffer(b, np.float32, p.channels * n, at).reshape(p.channels, n)
                    at += 4 * p.channels * n
                    rows = np.frombuffer(b, np.float32, n * p.outputs, at)
                    at += 4 * n * p.outputs
                    S.assert_bits(want_ch, ch, f"step {k}: oracle (got) against reference (want), channels of system {si} emitter {ei}")
                    S.assert_bits(want_rows, rows, f"step {k}: oracle (got) against reference (want), slice of system {si} emitter {ei}")
                    g += 1
        assert at == len(b)


@pytest.fixture
def as_reference(ref_exe, monkeypatch):
    RefPair.exe = ref_exe
    monkeypatch.setattr(S, "Pair", RefPair)


@pytest.mark.parametrize("n", [0, 1, 5, 65, 1023, 1025, 2049, 5 * 1024 + 1])
def test_counts(as_reference, n):
    S.test_counts(None, n)


def test_instructions(as_reference):
    S.test_whole_chunk_instructions(None)
    S.test_block_instructions(None)


@pytest.mark.parametrize("case", sorted(S.KILL_CASES))
def test_kills(as_reference, case):
    S.test_kills(None, case)


def test_kill_orders(as_reference):
    S.test_kill_in_the_padded_four(None)
    S.test_two_blocks_that_kill(None)
    S.test_cmp_else_kills_in_the_false_arm(None)
    S.test_block_writes_a_channel_and_then_kills(None)


def test_emission(as_reference):
    S.test_init_emit_count_on_the_first_step_only(None)
    for dt in (0.004, 0.01, 0.025, 0.3):
        S.test_emit_per_second(None, dt)


def test_sub_emission(as_reference):
    for records in (0, 1, 1025):
        S.test_sub_emission_into_a_later_emitter(None, records)
    S.test_sub_emission_into_an_earlier_emitter(None)
    S.test_sub_emission_chain_of_three(None, [8192, 8192, 8192])  # (the small capacities overflow: a case for the device alone)


def test_generated_systems(as_reference):
    rng = np.random.default_rng(17)
    systems = [[S.generated_program(rng) for _ in range(3)] for _ in range(40)]
    S.run(None, systems, 64, [float(x) for x in np.random.default_rng(5).uniform(0.01, 0.12, 20)], globals_=[0.125], positions=rng.uniform(-50.0, 50.0, (40, 3)))


def test_sin_cos_programs(as_reference):
    """the oracle calls the same libm as the compiled reference: bit-equal there too"""
    from tests import particle_asm as A
    from tests.particle_asm import CH, REG, LIT, SYS, OUT

    emit = [A.mul(CH(0), SYS(A.EMIT_INDEX), LIT(0.37)), A.sub(CH(0), CH(0), LIT(40.0))]
    update = [A.sin(CH(1), CH(0)), A.cos(CH(2), CH(0)), A.gt(REG(0), CH(0), LIT(-1.0e9)), A.cmp(REG(0), [A.sin(CH(3), CH(0)), A.cos(CH(4), CH(0))])]
    p = A.Program(update, emit, [A.sin(OUT(0), CH(0)), A.cos(OUT(1), CH(0))], channels=5, registers=1, outputs=2, init_emit_count=300)
    S.run(None, [[p]], 300, [0.1])


def test_rand_formula_against_random_generator(ref_exe):
    """RandomGenerator::randFloat(from, to) and the oracle's formula fed the same u32 (the generator's next rand(), core/math.cpp:1337-1341)"""
    exe, _ = ref_exe
    rng = np.random.default_rng(11)
    for _ in range(40):
        u, v = (int(x) for x in rng.integers(1, 2 ** 32, 2))
        lo, hi = float(np.float32(rng.uniform(-100, 100))), float(np.float32(rng.uniform(-100, 100)))
        u1 = (36969 * (u & 65535) + (u >> 16)) & 0xFFFFFFFF
        v1 = (18000 * (v & 65535) + (v >> 16)) & 0xFFFFFFFF
        r = ((u1 << 16) + v1) & 0xFFFFFFFF
        out = subprocess.run([exe, "rand", str(u), str(v), repr(lo), repr(hi)], check=True, capture_output=True, text=True).stdout
        assert int(out) == int(np.float32(O.rand_float(lo, hi, r)).view(np.uint32)), (u, v, lo, hi)
