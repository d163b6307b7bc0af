// lmx_capi_particles.hip — particle-system entry points (include/lumix_mi355.h, "particle systems" section): the registered systems and
// their decoded programs, the buffer layout, the host's scalar emission state (emit_timer, total time) and the launch chain of
// particle_kernels.hip. lmx_particles_step and lmx_particles_fill enqueue and return: no particle count reaches the host inside a step.
#include "lmx_context.h"
#include "lmx_particles.h"

using namespace lmx;

namespace {
constexpr uint32_t PARTICLES_MAGIC = 0x50415254u; // "PART": an object of another kind passed as LmxParticles is refused, not used
constexpr uint32_t MAX_CAPACITY = 1u << 26;
}

struct LmxParticles {
	uint32_t magic = PARTICLES_MAGIC;
	LmxContext* ctx = nullptr;
	struct Emitter {
		ParticleProgram prog;
		bool has_program = false;
		uint32_t channels = 0, registers = 0, outputs = 0, emit_inputs = 0, init_emit_count = 0, capacity = 0;
		float emit_per_second = 0.0f;
		float emit_timer = 0.0f; // Emitter::emit_timer: host state, it depends on dt alone
		// lmx_particles_set_emitter_options; an emitter that never got any is a non-ribbon emitter without emission on movement
		LmxParticleEmitterOptions opts = {0, 0, 0, 0, 0.0f};
		uint32_t ribbon_len = 0; // max_ribbon_length rounded up to a multiple of four
		struct Ribbon { uint32_t offset, length, emit_index, ring; }; // Emitter::ribbons, and the physical ring each keeps for life
		std::vector<Ribbon> ribbons;
		std::vector<uint32_t> free_rings; // taken from the back
		double last_emit_point[3] = {0, 0, 0}; // (the reference's Emitter gives it no initial value and reset() leaves it alone)
		bool is_ribbon() const { return opts.max_ribbons > 0; }
	};
	struct System {
		uint32_t first = 0, n = 0;
		std::vector<float> globals;
		double pos[3] = {0, 0, 0};
		float total_time = 0.0f; // ParticleSystem::m_total_time
		// what MESH / SPLINE read. A declaration, "none" included, is what lets set_program accept the instruction
		bool mesh_declared = false, spline_declared = false;
		LmxParticleMeshSource source = {PARTICLE_NO_SOURCE, PARTICLE_NO_SOURCE, 0};
		std::vector<float> spline; // xyz per point; empty: no spline component
	};
	struct Mesh { uint32_t vert_at, n_verts, skin_at; }; // skin_at = PARTICLE_NO_SOURCE: no skin
	std::vector<Mesh> meshes; // shared between the systems
	std::vector<float> mesh_positions;
	std::vector<LmxSkin> mesh_skins;
	bool meshes_changed = false, splines_changed = false; // the device arrays are older than the host's
	bool any_source = false; // a system has declared a source: until then the table is all "none" and a call has nothing to resolve
	std::vector<ParticleSourceDev> src_host, src_up[2]; // the table the device holds; what a call uploads (as sys_up)
	std::vector<float> spline_up[2];
	std::vector<System> systems;
	std::vector<Emitter> emitters;
	bool dirty = true; // the device tables and buffers are older than the registered programs / capacities
	uint32_t seed = 0, step = 0;
	uint32_t max_chunks = 0, max_registers = 0, max_shadow = 0, frame_floats = 0;
	uint32_t max_groups = 0, n_ribbon_emitters = 0, ribbon_slots = 0; // 1024-lane blocks of the largest ribbon emitter; ribbon emitters; the sum of their max_ribbons
	bool ribbons_changed = false; // a ring, a length or a row differs from what the device table holds
	uint32_t uploads = 0;  // calls that uploaded so far: call k uses set k & 1
	uint32_t levels = 0;   // the largest number of emitters in one system
	bool any_emit = false; // a program holds EMIT: emitter k of every system is updated and drained before emitter k + 1 (one pass per k)
	std::vector<ParticleEmitterDev> table;
	// what a step uploads, twice: a step fills the set the step before the last one used, once that one's copies have left the host
	// (uploaded[set], recorded behind them) - lmx_particles_step never waits for the kernels of an earlier step
	std::vector<ParticleSystemDev> sys_host, sys_up[2];
	std::vector<ParticleEmitJob> jobs_first_up[2], jobs_rate_up[2];
	std::vector<ParticleRibbonJob> rjobs_first_up[2], rjobs_rate_up[2];
	std::vector<ParticleRibbonDev> ribbons_up[2];
	std::vector<ParticleRibbonCount> ribbon_counts_up[2];
	hipEvent_t uploaded[2] = {nullptr, nullptr};
	bool upload_pending[2] = {false, false};
	~LmxParticles() {
		for (hipEvent_t e : uploaded)
			if (e) (void)hipEventDestroy(e);
	}
	DevBuf<ParticleEmitterDev> d_emitters;
	DevBuf<ParticleSystemDev> d_systems;
	DevBuf<ParticleRec> d_prog;
	DevBuf<ParticleGradient> d_gradients;
	DevBuf<float> d_globals, d_channels, d_frame;
	DevBuf<ParticleStateDev> d_state;
	DevBuf<uint32_t> d_kill, d_n_ops, d_stage, d_n_sub;
	DevBuf<ParticleSubJob> d_sub_jobs;
	DevBuf<ParticleCopyOp> d_ops;
	DevBuf<LmxParticleSlice> d_slices;
	DevBuf<ParticleEmitJob> d_jobs_first, d_jobs_rate;
	DevBuf<ParticleRibbonJob> d_rjobs_first, d_rjobs_rate;
	DevBuf<ParticleRibbonDev> d_ribbons;
	DevBuf<ParticleRibbonCount> d_ribbon_counts;
	DevBuf<ParticleSourceDev> d_sources;
	DevBuf<float> d_mesh_positions, d_spline;
	DevBuf<LmxSkin> d_mesh_skins;

	ParticlesDevice dev() const {
		ParticlesDevice d;
		d.emitters = d_emitters.p; d.systems = d_systems.p; d.prog = d_prog.p; d.gradients = d_gradients.p; d.globals = d_globals.p;
		d.channels = d_channels.p; d.state = d_state.p; d.kill = d_kill.p; d.ops = d_ops.p; d.n_ops = d_n_ops.p; d.slices = d_slices.p; d.frame = d_frame.p;
		d.stage = d_stage.p; d.sub_jobs = d_sub_jobs.p; d.n_sub = d_n_sub.p; d.level = 0xffffffffu;
		d.ribbons = d_ribbons.p; d.ribbon_counts = d_ribbon_counts.p; d.n_ribbon_emitters = n_ribbon_emitters;
		d.sources = d_sources.p; d.mesh_positions = d_mesh_positions.p; d.mesh_skins = d_mesh_skins.p; d.spline_points = d_spline.p;
		d.palette = ctx->skin.d_palette.p;
		d.n_emitters = (uint32_t)emitters.size(); d.seed = seed; d.step = step; d.frame_floats = frame_floats;
		return d;
	}
};

static_assert(sizeof(LmxParticlesCounts) == sizeof(ParticleStateDev), "lmx_particles_counts reads the state records as they are");

namespace {

#define LMX_CHECK_PARTICLES(ps)                                                         \
	if ((ps) && (ps)->magic != PARTICLES_MAGIC) return LMX_ERR_INVALID_ARGUMENT;       \
	LMX_ENTER(ps)

int find_emitter(LmxParticles* ps, uint32_t system, uint32_t emitter, uint32_t* out) {
	if (system >= ps->systems.size()) return fail(ps->ctx, LMX_ERR_INVALID_ARGUMENT, "particle system %u: %zu registered", system, ps->systems.size());
	if (emitter >= ps->systems[system].n) return fail(ps->ctx, LMX_ERR_INVALID_ARGUMENT, "emitter %u: system %u has %u", emitter, system, ps->systems[system].n);
	*out = ps->systems[system].first + emitter;
	return LMX_OK;
}

void reset_host(LmxParticles* ps, uint32_t system) {
	LmxParticles::System& s = ps->systems[system];
	s.total_time = 0.0f;
	for (uint32_t e = s.first; e < s.first + s.n; ++e) {
		LmxParticles::Emitter& em = ps->emitters[e];
		em.emit_timer = 0.0f;
		// (the reference's reset() zeroes particles_count and keeps Emitter::ribbons, whose lengths then no longer add up to it: here a
		// reset system has no ribbons, and its first frame emits init_ribbons_count again)
		if (!em.ribbons.empty()) ps->ribbons_changed = true;
		em.ribbons.clear();
		em.free_rings.resize(em.opts.max_ribbons);
		for (uint32_t r = 0; r < em.opts.max_ribbons; ++r) em.free_rings[r] = em.opts.max_ribbons - 1 - r;
	}
}

// A call that uploads takes the set the call before the last one used, once that call's copies have left the host (uploaded[set], recorded
// behind them): no call waits for the kernels of an earlier one.
int begin_upload(LmxParticles* ps, uint32_t* out_set) {
	LmxContext* ctx = ps->ctx;
	const uint32_t set = ps->uploads & 1u;
	if (!ps->uploaded[set]) LMX_HIP(ctx, hipEventCreateWithFlags(&ps->uploaded[set], hipEventDisableTiming));
	if (ps->upload_pending[set]) LMX_HIP(ctx, hipEventSynchronize(ps->uploaded[set]));
	ps->upload_pending[set] = false;
	ps->jobs_first_up[set].clear(); ps->jobs_rate_up[set].clear();
	ps->rjobs_first_up[set].clear(); ps->rjobs_rate_up[set].clear();
	*out_set = set;
	return LMX_OK;
}

int end_upload(LmxParticles* ps, uint32_t set) {
	LmxContext* ctx = ps->ctx;
	LMX_HIP(ctx, hipEventRecord(ps->uploaded[set], ctx->stream));
	ps->upload_pending[set] = true;
	++ps->uploads;
	return LMX_OK;
}

// ParticleSystem::emitRibbonPoints, the integer part: the job carries the ribbon as it was, the ribbon moves on
void emit_points_host(LmxParticles* ps, uint32_t e, uint32_t ribbon, uint32_t count, float total_time, float time_step, std::vector<ParticleRibbonJob>& jobs, uint32_t& lanes) {
	LmxParticles::Emitter& em = ps->emitters[e];
	LmxParticles::Emitter::Ribbon& rb = em.ribbons[ribbon];
	if (!count) return;
	jobs.push_back(ParticleRibbonJob{e, ribbon, rb.ring, rb.offset, rb.length, rb.emit_index, count, lanes, total_time, time_step});
	lanes += std::min(count, em.ribbon_len);
	const uint32_t room = em.ribbon_len - rb.length;
	if (room) ps->ribbons_changed = true;
	if (count <= room) {
		rb.length += count;
	} else {
		rb.length = em.ribbon_len;
		rb.offset += count - room; // the reference's unbounded u32
	}
	rb.emit_index += count;
}

// ParticleSystem::emitRibbons (:1597-1618)
void emit_ribbons_host(LmxParticles* ps, uint32_t e, uint32_t n, float total_time, std::vector<ParticleRibbonJob>& jobs, uint32_t& lanes) {
	LmxParticles::Emitter& em = ps->emitters[e];
	n = std::min<uint32_t>(n, em.opts.max_ribbons - (uint32_t)em.ribbons.size());
	for (uint32_t k = 0; k < n; ++k) {
		const uint32_t ring = em.free_rings.back();
		em.free_rings.pop_back();
		em.ribbons.push_back(LmxParticles::Emitter::Ribbon{0, 0, 0, ring});
		ps->ribbons_changed = true;
		emit_points_host(ps, e, (uint32_t)em.ribbons.size() - 1, em.init_emit_count, total_time, 0.0f, jobs, lanes);
	}
}

// The device's ribbon table and the ribbon emitters' counts, when a call changed them; then Emitter::particles_count into the state records
int upload_ribbons(LmxParticles* ps, uint32_t set) {
	LmxContext* ctx = ps->ctx;
	if (!ps->n_ribbon_emitters || !ps->ribbons_changed) return LMX_OK;
	std::vector<ParticleRibbonDev>& tab = ps->ribbons_up[set];
	std::vector<ParticleRibbonCount>& cnt = ps->ribbon_counts_up[set];
	tab.assign(ps->ribbon_slots, ParticleRibbonDev{0, 0, 0, 0});
	cnt.assign(ps->n_ribbon_emitters, ParticleRibbonCount{0, 0, 0, 0});
	for (uint32_t e = 0; e < ps->emitters.size(); ++e) {
		const LmxParticles::Emitter& em = ps->emitters[e];
		if (!em.is_ribbon()) continue;
		const ParticleEmitterDev& t = ps->table[e];
		uint32_t row = 0;
		for (size_t r = 0; r < em.ribbons.size(); ++r) {
			tab[t.ribbon_base + r] = ParticleRibbonDev{em.ribbons[r].ring, em.ribbons[r].length, row, 0};
			row += em.ribbons[r].length;
		}
		cnt[t.ribbon_ord] = ParticleRibbonCount{e, (uint32_t)em.ribbons.size(), row, 0};
	}
	LMX_HIP(ctx, upload_on_stream(ps->d_ribbons.p, tab.data(), tab.size(), ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_ribbon_counts.p, cnt.data(), cnt.size(), ctx->stream));
	LMX_HIP(ctx, launch_particles_ribbon_commit(ctx->stream, ps->dev()));
	ps->ribbons_changed = false;
	return LMX_OK;
}

// The per-system source records as this moment's host state gives them: the mesh and spline tables, and the palette the last lmx_skin_run
// left for the declared skin instance (read as k_ray_narrow reads it: the instance's bone range of the one palette buffer).
int resolve_sources(LmxParticles* ps, std::vector<ParticleSourceDev>& out) {
	LmxContext* ctx = ps->ctx;
	const SkinState& sk = ctx->skin;
	out.assign(ps->systems.size(), ParticleSourceDev{0, 0, PARTICLE_NO_SOURCE, PARTICLE_NO_SOURCE, 0, 0, 0, 0});
	uint32_t spline_at = 0;
	for (size_t s = 0; s < ps->systems.size(); ++s) {
		const LmxParticles::System& sy = ps->systems[s];
		ParticleSourceDev& r = out[s];
		r.spline_at = spline_at;
		r.n_points = (uint32_t)(sy.spline.size() / 3);
		spline_at += r.n_points;
		if (!sy.mesh_declared) continue;
		if (sy.source.mesh != PARTICLE_NO_SOURCE) { // (< meshes.size(): checked by the setter, reset by clear_meshes)
			const LmxParticles::Mesh& m = ps->meshes[sy.source.mesh];
			r.mesh_at = m.vert_at; r.n_verts = m.n_verts; r.skin_at = m.skin_at;
		}
		r.flags = sy.source.flags & PARTICLE_SOURCE_BONES;
		if (sy.source.skin_instance != PARTICLE_NO_SOURCE) {
			if (!sk.palette_valid || !sk.d_palette.p) return fail(ctx, LMX_ERR_NOT_BUILT, "particle system %zu reads the pose of skin instance %u: no lmx_skin_run has left a palette", s, sy.source.skin_instance);
			if (sy.source.skin_instance >= sk.inst.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "particle system %zu reads the pose of skin instance %u: the skinning module has %zu", s, sy.source.skin_instance, sk.inst.size());
			r.palette_at = sk.inst[sy.source.skin_instance].bone_offset;
			r.n_bones = sk.inst[sy.source.skin_instance].n_bones;
		}
	}
	return LMX_OK;
}

// Uploads what of the source tables changed, inside a begin_upload / end_upload pair (`set`): in stream order, no buffer of the particles is
// touched. The mesh arrays change only when a mesh is added or all are cleared: that copy is waited for.
int upload_sources(LmxParticles* ps, uint32_t set, const std::vector<ParticleSourceDev>& now) {
	LmxContext* ctx = ps->ctx;
	if (ps->meshes_changed) {
		LMX_HIP(ctx, upload_on_stream(ps->d_mesh_positions, ps->mesh_positions, ctx->stream));
		LMX_HIP(ctx, upload_on_stream(ps->d_mesh_skins, ps->mesh_skins, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		ps->meshes_changed = false;
	}
	if (ps->splines_changed) {
		std::vector<float>& up = ps->spline_up[set];
		up.clear();
		for (const LmxParticles::System& sy : ps->systems) up.insert(up.end(), sy.spline.begin(), sy.spline.end());
		LMX_HIP(ctx, upload_on_stream(ps->d_spline, up, ctx->stream));
		ps->splines_changed = false;
	}
	if (now.size() != ps->src_host.size() || (!now.empty() && memcmp(now.data(), ps->src_host.data(), now.size() * sizeof(ParticleSourceDev)) != 0)) {
		ps->src_up[set] = now;
		LMX_HIP(ctx, upload_on_stream(ps->d_sources, ps->src_up[set], ctx->stream));
		ps->src_host = now;
	}
	return LMX_OK;
}
// nothing declared anywhere and the device holds the all-"none" table of this many systems: a step or fill spends nothing on the sources
bool sources_quiet(const LmxParticles* ps) {
	return !ps->any_source && !ps->meshes_changed && !ps->splines_changed && ps->src_host.size() == ps->systems.size();
}
bool sources_stale(const LmxParticles* ps, const std::vector<ParticleSourceDev>& now) {
	return ps->meshes_changed || ps->splines_changed || now.size() != ps->src_host.size() ||
	       (!now.empty() && memcmp(now.data(), ps->src_host.data(), now.size() * sizeof(ParticleSourceDev)) != 0);
}

// ... for a call that runs programs and has no upload of its own to put them in
int sync_sources(LmxParticles* ps) {
	if (sources_quiet(ps)) return LMX_OK;
	std::vector<ParticleSourceDev> now;
	if (int rc = resolve_sources(ps, now)) return rc;
	if (!sources_stale(ps, now)) return LMX_OK;
	uint32_t set;
	if (int rc = begin_upload(ps, &set)) return rc;
	if (int rc = upload_sources(ps, set, now)) return rc;
	return end_upload(ps, set);
}

// What a ribbon emitter's program may not hold (include/lumix_mi355.h): checked by whichever of set_program / set_emitter_options comes later
int check_ribbon_program(LmxContext* ctx, const ParticleProgram& prog) {
	if (prog.has_kill) return fail(ctx, LMX_ERR_INVALID, "KILL in a ribbon emitter's update program: updateRibbons has no kill counter to write it to");
	if (prog.has_emit) return fail(ctx, LMX_ERR_UNSUPPORTED, "EMIT in a ribbon emitter's update program: ribbon sub-emission is not run on the device");
	return LMX_OK;
}

// Device tables, program records and buffers for the registered programs and capacities. Everything starts empty: a new layout is a reset.
int build(LmxParticles* ps) {
	LmxContext* ctx = ps->ctx;
	for (size_t e = 0; e < ps->emitters.size(); ++e)
		if (!ps->emitters[e].has_program) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_particles_set_program has not been called for every emitter (global emitter %zu)", e);
	if (!ps->dirty) return LMX_OK;
	for (const LmxParticles::System& sy : ps->systems) // needs another emitter's options: no call before this one can know
		for (uint32_t k = 0; k < sy.n; ++k) {
			const LmxParticles::Emitter& em = ps->emitters[sy.first + k];
			for (uint32_t j = 0; j < em.prog.emit_count; ++j)
				if (ps->emitters[sy.first + em.prog.emit_target[j]].is_ribbon())
					return fail(ctx, LMX_ERR_INVALID, "emitter %u of a system has an EMIT into its ribbon emitter %u: the reference drains it as if the rings were one flat array", k, em.prog.emit_target[j]);
		}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	const size_t n = ps->emitters.size();
	ps->max_groups = ps->n_ribbon_emitters = ps->ribbon_slots = 0;
	std::vector<ParticleRec> recs;
	std::vector<ParticleGradient> grads;
	std::vector<float> globals;
	ps->table.assign(n, ParticleEmitterDev());
	ps->sys_host.assign(ps->systems.size(), ParticleSystemDev());
	uint64_t floats = 0, frame = 0, stage_words = 0, sub_jobs = 0;
	uint32_t chunks_total = 0;
	ps->levels = 0;
	ps->any_emit = false;
	ps->max_chunks = ps->max_registers = ps->max_shadow = 0;
	for (size_t s = 0; s < ps->systems.size(); ++s) {
		LmxParticles::System& sy = ps->systems[s];
		memset(&ps->sys_host[s], 0, sizeof(ParticleSystemDev));
		ps->sys_host[s].globals_at = (uint32_t)globals.size();
		ps->sys_host[s].n_globals = (uint32_t)sy.globals.size();
		globals.insert(globals.end(), sy.globals.begin(), sy.globals.end());
		for (uint32_t k = 0; k < sy.n; ++k) {
			const LmxParticles::Emitter& em = ps->emitters[sy.first + k];
			ParticleEmitterDev& t = ps->table[sy.first + k];
			memset(&t, 0, sizeof(t));
			const uint32_t base = (uint32_t)recs.size(), gbase = (uint32_t)grads.size();
			for (ParticleRec r : em.prog.recs) { // record indices become absolute
				if (r.op == P_CMP || r.op == P_CMP_ELSE) { r.a += base; r.c += base; }
				if (r.op == P_END && r.kind == PE_JUMP) r.a += base;
				if (r.op == P_GRADIENT) r.a += gbase;
				recs.push_back(r);
			}
			grads.insert(grads.end(), em.prog.gradients.begin(), em.prog.gradients.end());
			t.system = (uint32_t)s;
			t.prog_update = base + em.prog.update_at; t.prog_emit = base + em.prog.emit_at; t.prog_output = base + em.prog.output_at;
			t.channels = em.channels; t.registers = em.registers; t.outputs = em.outputs; t.emit_inputs = em.emit_inputs;
			t.capacity = em.capacity;
			t.stride = em.capacity + PARTICLE_GUARD_FLOATS;
			t.max_chunks = (em.capacity + PARTICLE_CHUNK - 1) / PARTICLE_CHUNK;
			if (em.is_ribbon()) { // capacity = max_ribbons x ribbon_len (set_emitter_options): its points are k_particles_ribbon_chunk's
				t.ribbon_len = em.ribbon_len; t.max_ribbons = em.opts.max_ribbons;
				t.ribbon_base = ps->ribbon_slots; t.ribbon_ord = ps->n_ribbon_emitters++;
				ps->ribbon_slots += em.opts.max_ribbons;
				const uint32_t per = PARTICLE_CHUNK / em.ribbon_len;
				ps->max_groups = std::max(ps->max_groups, (em.opts.max_ribbons + per - 1) / per);
			}
			t.shadow_mask = em.prog.shadow_mask;
			t.channel_base = floats;
			t.kill_base = chunks_total;
			t.local = k; t.first_of_system = sy.first; t.init_emit_count = em.init_emit_count;
			t.n_emit = em.prog.emit_count;
			memcpy(t.emit_group, em.prog.emit_group, sizeof(t.emit_group));
			t.stage_base = stage_words;
			t.job_base = (uint32_t)sub_jobs;
			stage_words += (uint64_t)em.capacity * t.n_emit * PARTICLE_STAGE_WORDS;
			sub_jobs += (uint64_t)em.capacity * t.n_emit;
			ps->any_emit = ps->any_emit || t.n_emit != 0;
			ps->levels = std::max(ps->levels, k + 1);
			floats += (uint64_t)t.stride * em.channels;
			frame += (uint64_t)em.capacity * em.outputs;
			chunks_total += t.max_chunks;
			if (!em.is_ribbon()) ps->max_chunks = std::max(ps->max_chunks, t.max_chunks);
			ps->max_registers = std::max(ps->max_registers, em.registers);
			ps->max_shadow = std::max(ps->max_shadow, (uint32_t)__builtin_popcount(em.prog.shadow_mask));
		}
	}
	if (sub_jobs > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "the sub-emission staging of every emitter at capacity exceeds 2^32 records");
	if (frame * 4 + PARTICLE_GUARD_FLOATS * 4 > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "the frame buffer of every emitter at capacity exceeds 4 GiB");
	ps->frame_floats = (uint32_t)frame;
	LMX_HIP(ctx, upload_on_stream(ps->d_emitters, ps->table, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_prog, recs, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_gradients, grads, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_globals, globals, ctx->stream));
	LMX_HIP(ctx, ps->d_systems.reserve(std::max<size_t>(ps->systems.size(), 1)));
	LMX_HIP(ctx, ps->d_channels.reserve(std::max<size_t>(floats, 1)));
	LMX_HIP(ctx, ps->d_frame.reserve(frame + PARTICLE_GUARD_FLOATS));
	LMX_HIP(ctx, ps->d_state.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, ps->d_kill.reserve(std::max<uint32_t>(chunks_total, 1)));
	LMX_HIP(ctx, ps->d_ops.reserve(std::max<uint32_t>(chunks_total, 1)));
	LMX_HIP(ctx, ps->d_n_ops.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, ps->d_n_sub.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, ps->d_stage.reserve(std::max<uint64_t>(stage_words, 1)));
	LMX_HIP(ctx, ps->d_sub_jobs.reserve(std::max<uint64_t>(sub_jobs, 1)));
	LMX_HIP(ctx, ps->d_slices.reserve(std::max<size_t>(n, 1)));
	LMX_HIP(ctx, ps->d_ribbons.reserve(std::max<uint32_t>(ps->ribbon_slots, 1)));
	LMX_HIP(ctx, ps->d_ribbon_counts.reserve(std::max<uint32_t>(ps->n_ribbon_emitters, 1)));
	LMX_HIP(ctx, upload_on_stream(ps->d_systems.p, ps->sys_host.data(), ps->sys_host.size(), ctx->stream)); // (emit_ribbons / apply_transforms before the first step)
	LMX_HIP(ctx, hipMemsetAsync(ps->d_channels.p, 0, floats * sizeof(float), ctx->stream));
	for (size_t e = 0; e < n; ++e) { // the guards behind every channel
		const ParticleEmitterDev& t = ps->table[e];
		for (uint32_t c = 0; c < t.channels; ++c)
			LMX_HIP(ctx, fill_guard(ps->d_channels.p + t.channel_base + (size_t)c * t.stride + t.capacity, PARTICLE_GUARD_FLOATS, ctx->stream));
	}
	LMX_HIP(ctx, hipMemsetAsync(ps->d_frame.p, 0, frame * sizeof(float), ctx->stream));
	LMX_HIP(ctx, fill_guard(ps->d_frame.p + frame, PARTICLE_GUARD_FLOATS, ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_state.p, 0, std::max<size_t>(n, 1) * sizeof(ParticleStateDev), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_kill.p, 0, std::max<uint32_t>(chunks_total, 1) * sizeof(uint32_t), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_n_ops.p, 0, std::max<size_t>(n, 1) * sizeof(uint32_t), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_n_sub.p, 0, std::max<size_t>(n, 1) * sizeof(uint32_t), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_stage.p, 0, std::max<uint64_t>(stage_words, 1) * sizeof(uint32_t), ctx->stream));
	LMX_HIP(ctx, hipMemsetAsync(ps->d_slices.p, 0, std::max<size_t>(n, 1) * sizeof(LmxParticleSlice), ctx->stream));
	for (uint32_t s = 0; s < ps->systems.size(); ++s) reset_host(ps, s);
	ps->ribbons_changed = true; // the table of a world without ribbons, from arrays that outlive the copies
	if (int rc = upload_ribbons(ps, 0)) return rc;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ps->step = 0;
	ps->dirty = false;
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_particles_create(LmxContext* ctx, LmxParticles** out) { return object_create(ctx, out, "particles"); }

void lmx_particles_destroy(LmxParticles* ps) {
	if (!ps || ps->magic != PARTICLES_MAGIC) return;
	ps->magic = 0;
	object_destroy(ps);
}

int lmx_particles_add_system(LmxParticles* ps, uint32_t n_emitters, uint32_t n_globals, uint32_t* out_system) {
	LMX_CHECK_PARTICLES(ps);
	if (n_globals > 256) return fail(ctx, LMX_ERR_CAPACITY, "%u globals: a program's operand indexes at most 256", n_globals);
	if (n_emitters > 65536 || ps->emitters.size() + n_emitters > 65535) return fail(ctx, LMX_ERR_CAPACITY, "more than 65535 emitters (a launch's grid)");
	LmxParticles::System s;
	s.first = (uint32_t)ps->emitters.size();
	s.n = n_emitters;
	s.globals.assign(n_globals, 0.0f);
	ps->emitters.resize(ps->emitters.size() + n_emitters);
	if (out_system) *out_system = (uint32_t)ps->systems.size();
	ps->systems.push_back(std::move(s));
	ps->dirty = true;
	return LMX_OK;
}

int lmx_particles_set_program(LmxParticles* ps, uint32_t system, uint32_t emitter, const LmxParticleProgram* p) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (!p || !p->instructions) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null program");
	ParticleProgramDesc desc;
	desc.bytes = p->instructions; desc.size = p->size; desc.emit_offset = p->emit_offset; desc.output_offset = p->output_offset;
	desc.channels_count = p->channels_count; desc.registers_count = p->registers_count; desc.outputs_count = p->outputs_count;
	desc.emit_inputs_count = p->emit_inputs_count;
	desc.n_emitters = ps->systems[system].n;
	desc.n_globals = (uint32_t)ps->systems[system].globals.size();
	desc.sources = (ps->systems[system].mesh_declared ? PARTICLE_SRC_MESH : 0u) | (ps->systems[system].spline_declared ? PARTICLE_SRC_SPLINE : 0u);
	ParticleProgram prog;
	std::string err;
	const ParticleDecodeResult decoded = particle_program_decode(desc, prog, err);
	if (decoded != PD_OK) return fail(ctx, decoded == PD_UNSUPPORTED ? LMX_ERR_UNSUPPORTED : LMX_ERR_INVALID, "%s", err.c_str());
	if (prog.stopped) return fail(ctx, LMX_ERR_UNSUPPORTED, "MESH / SPLINE instructions need the entity's mesh, pose and spline: not run on the device");
	if (!(p->emit_per_second == p->emit_per_second)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "emit_per_second is not a number");
	LmxParticles::Emitter& em = ps->emitters[e];
	if (em.is_ribbon())
		if (int rc = check_ribbon_program(ctx, prog)) return rc;
	em.prog = std::move(prog);
	em.has_program = true;
	em.channels = p->channels_count; em.registers = p->registers_count; em.outputs = p->outputs_count; em.emit_inputs = p->emit_inputs_count;
	em.init_emit_count = p->init_emit_count;
	em.emit_per_second = p->emit_per_second;
	ps->dirty = true;
	return LMX_OK;
}

int lmx_particles_set_globals(LmxParticles* ps, uint32_t system, const float* globals, uint32_t n) {
	LMX_CHECK_PARTICLES(ps);
	if (system >= ps->systems.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "particle system %u: %zu registered", system, ps->systems.size());
	LmxParticles::System& s = ps->systems[system];
	if (n != s.globals.size() || (n && !globals)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "system %u has %zu globals", system, s.globals.size());
	if (n) memcpy(s.globals.data(), globals, n * sizeof(float));
	if (!ps->dirty && n) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		LMX_HIP(ctx, upload_on_stream(ps->d_globals.p + ps->sys_host[system].globals_at, s.globals.data(), n, ctx->stream)); // (the system's own array: it stays)
	}
	return LMX_OK;
}

int lmx_particles_set_entity_positions(LmxParticles* ps, uint32_t n_systems, const double* pos_xyz) {
	LMX_CHECK_PARTICLES(ps);
	if (n_systems != ps->systems.size() || (n_systems && !pos_xyz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%zu particle systems registered", ps->systems.size());
	for (uint32_t s = 0; s < n_systems; ++s) memcpy(ps->systems[s].pos, pos_xyz + 3 * (size_t)s, sizeof(double) * 3);
	return LMX_OK;
}

int lmx_particles_reserve(LmxParticles* ps, uint32_t system, uint32_t emitter, uint32_t capacity) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (capacity > MAX_CAPACITY) return fail(ctx, LMX_ERR_CAPACITY, "%u particles: at most 2^26 per emitter", capacity);
	if (ps->emitters[e].is_ribbon()) return fail(ctx, LMX_ERR_INVALID, "a ribbon emitter's capacity is max_ribbons x max_ribbon_length");
	ps->emitters[e].capacity = (capacity + 3u) & ~3u;
	ps->dirty = true;
	return LMX_OK;
}

int lmx_particles_reset(LmxParticles* ps, uint32_t system) {
	LMX_CHECK_PARTICLES(ps);
	if (system != 0xffffffffu && system >= ps->systems.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "particle system %u: %zu registered", system, ps->systems.size());
	const uint32_t s0 = system == 0xffffffffu ? 0 : system, s1 = system == 0xffffffffu ? (uint32_t)ps->systems.size() : system + 1;
	for (uint32_t s = s0; s < s1; ++s) {
		reset_host(ps, s);
		if (!ps->dirty && ps->systems[s].n)
			LMX_HIP(ctx, hipMemsetAsync(ps->d_state.p + ps->systems[s].first, 0, ps->systems[s].n * sizeof(ParticleStateDev), ctx->stream));
	}
	if (!ps->dirty && ps->ribbons_changed) { // the ribbons that went
		uint32_t set;
		if (int rc = begin_upload(ps, &set)) return rc;
		if (int rc = upload_ribbons(ps, set)) return rc;
		if (int rc = end_upload(ps, set)) return rc;
	}
	return LMX_OK;
}

int lmx_particles_set_seed(LmxParticles* ps, uint32_t seed) {
	LMX_CHECK_PARTICLES(ps);
	ps->seed = seed;
	return LMX_OK;
}

int lmx_particles_step(LmxParticles* ps, float dt) {
	LMX_CHECK_PARTICLES(ps);
	if (int rc = build(ps)) return rc;
	if (ps->emitters.empty()) return LMX_OK;
	std::vector<ParticleSourceDev> sources;
	const bool quiet = sources_quiet(ps);
	if (!quiet)
		if (int rc = resolve_sources(ps, sources)) return rc; // (before any host state moves: a refused step changes nothing)
	uint32_t set;
	if (int rc = begin_upload(ps, &set)) return rc;
	if (!quiet)
		if (int rc = upload_sources(ps, set, sources)) return rc;
	std::vector<ParticleEmitJob>&jobs_first = ps->jobs_first_up[set], &jobs_rate = ps->jobs_rate_up[set];
	std::vector<ParticleRibbonJob>&rjobs_first = ps->rjobs_first_up[set], &rjobs_rate = ps->rjobs_rate_up[set];
	uint32_t max_first = 0, max_rate = 0, lanes_first = 0, lanes_rate = 0;
	for (size_t s = 0; s < ps->systems.size(); ++s) { // ParticleSystem::update(dt, page_allocator), the scalar part
		LmxParticles::System& sy = ps->systems[s];
		ParticleSystemDev& sv = ps->sys_host[s];
		sv.values[PSV_TIME_DELTA] = dt;
		sv.values[PSV_EMIT_INDEX] = 0.0f;
		sv.values[PSV_RIBBON_INDEX] = 0.0f;
		sv.values[PSV_ENTITY_X] = (float)sy.pos[0]; sv.values[PSV_ENTITY_Y] = (float)sy.pos[1]; sv.values[PSV_ENTITY_Z] = (float)sy.pos[2];
		if (sy.total_time == 0.0f) {
			for (uint32_t e = sy.first; e < sy.first + sy.n; ++e) {
				const LmxParticles::Emitter& em = ps->emitters[e];
				if (em.is_ribbon()) {
					emit_ribbons_host(ps, e, em.opts.init_ribbons_count, sy.total_time, rjobs_first, lanes_first);
				} else if (em.emit_inputs == 0 && em.init_emit_count) {
					jobs_first.push_back(ParticleEmitJob{e, em.init_emit_count, sy.total_time, 0.0f});
					max_first = std::max(max_first, em.init_emit_count);
				}
			}
		}
		sy.total_time += dt;
		sv.values[PSV_TOTAL_TIME] = sy.total_time;
		for (uint32_t e = sy.first; e < sy.first + sy.n; ++e) { // the head of update(dt, emitter_idx, ...), :1467-1478
			LmxParticles::Emitter& em = ps->emitters[e];
			if (!(em.emit_per_second > 0)) continue;
			em.emit_timer += dt;
			if (!(em.emit_timer > 0)) continue;
			const float d = 1.f / em.emit_per_second;
			const float q = floorf(em.emit_timer / d);
			const uint32_t count = q < 9223372036854775808.0f ? (uint32_t)(uint64_t)(int64_t)q : 0u; // u32(float) as x86-64 converts it
			em.emit_timer -= d * count;
			if (!count) continue;
			if (em.is_ribbon()) { // updateRibbons (:1409-1421): `count` points into every ribbon
				for (uint32_t r = 0; r < em.ribbons.size(); ++r) emit_points_host(ps, e, r, count, sy.total_time, d, rjobs_rate, lanes_rate);
				continue;
			}
			jobs_rate.push_back(ParticleEmitJob{e, count, sy.total_time, d});
			max_rate = std::max(max_rate, count);
		}
	}
	ps->sys_up[set] = ps->sys_host;
	LMX_HIP(ctx, upload_on_stream(ps->d_systems, ps->sys_up[set], ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_jobs_first, jobs_first, ctx->stream));
	// (the rate jobs were pushed system by system: sorted by the emitter's index in its system, one pass takes a contiguous range)
	std::stable_sort(jobs_rate.begin(), jobs_rate.end(), [&](const ParticleEmitJob& a, const ParticleEmitJob& b) { return ps->table[a.emitter].local < ps->table[b.emitter].local; });
	LMX_HIP(ctx, upload_on_stream(ps->d_jobs_rate, jobs_rate, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_rjobs_first, rjobs_first, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_rjobs_rate, rjobs_rate, ctx->stream));
	++ps->step;
	if (int rc = upload_ribbons(ps, set)) return rc;
	if (int rc = end_upload(ps, set)) return rc;
	ParticlesDevice d = ps->dev();
	// Ribbon emitters depend on no other emitter and none depends on them (an EMIT into one is refused): all of them in one pass, whatever
	// their index in their system - the first frame's ribbons, the step's points, the update
	LMX_HIP(ctx, launch_particles_ribbon_emit(ctx->stream, d, ps->d_rjobs_first.p, (uint32_t)rjobs_first.size(), lanes_first));
	LMX_HIP(ctx, launch_particles_ribbon_emit(ctx->stream, d, ps->d_rjobs_rate.p, (uint32_t)rjobs_rate.size(), lanes_rate));
	LMX_HIP(ctx, launch_particles_ribbon_update(ctx->stream, d, ps->max_groups, ps->max_registers));
	const uint32_t cap_lanes = ps->max_chunks * PARTICLE_CHUNK; // a launch covers what fits the emitters' capacities: the rest of an oversized emission is only counted
	LMX_HIP(ctx, launch_particles_emit(ctx->stream, d, ps->d_jobs_first.p, (uint32_t)jobs_first.size(), std::min(max_first, cap_lanes)));
	if (!ps->any_emit) { // no emitter depends on another: one pass over all of them
		LMX_HIP(ctx, launch_particles_emit(ctx->stream, d, ps->d_jobs_rate.p, (uint32_t)jobs_rate.size(), std::min(max_rate, cap_lanes)));
		LMX_HIP(ctx, launch_particles_update(ctx->stream, d, ps->max_chunks, ps->max_registers, ps->max_shadow, false));
		return LMX_OK;
	}
	size_t at = 0;
	for (uint32_t k = 0; k < ps->levels; ++k) { // emitter k of every system: its rate emission, update, compaction, then the drain of its EMIT records
		size_t end = at;
		while (end < jobs_rate.size() && ps->table[jobs_rate[end].emitter].local == k) ++end;
		d.level = k;
		LMX_HIP(ctx, launch_particles_emit(ctx->stream, d, ps->d_jobs_rate.p + at, (uint32_t)(end - at), std::min(max_rate, cap_lanes)));
		LMX_HIP(ctx, launch_particles_update(ctx->stream, d, ps->max_chunks, ps->max_registers, ps->max_shadow, true));
		at = end;
	}
	return LMX_OK;
}

int lmx_particles_fill(LmxParticles* ps) {
	LMX_CHECK_PARTICLES(ps);
	if (int rc = build(ps)) return rc;
	if (ps->emitters.empty()) return LMX_OK;
	if (int rc = sync_sources(ps)) return rc;
	LMX_HIP(ctx, launch_particles_fill(ctx->stream, ps->dev(), ps->max_chunks, ps->max_registers));
	LMX_HIP(ctx, launch_particles_ribbon_fill(ctx->stream, ps->dev(), ps->max_groups, ps->max_registers));
	return LMX_OK;
}

int lmx_particles_counts(LmxParticles* ps, LmxParticlesCounts* out, uint32_t cap) {
	LMX_CHECK_PARTICLES(ps);
	if (int rc = build(ps)) return rc;
	if (cap < ps->emitters.size() || (!out && !ps->emitters.empty())) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu emitters", ps->emitters.size());
	return read_now(ctx, (ParticleStateDev*)out, (const ParticleStateDev*)ps->d_state.p, ps->emitters.size());
}

int lmx_particles_read_channels(LmxParticles* ps, uint32_t system, uint32_t emitter, float* out, uint32_t cap_floats, uint32_t* out_stride) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (int rc = build(ps)) return rc;
	const ParticleEmitterDev& t = ps->table[e];
	const size_t need = (size_t)t.stride * t.channels;
	if (out_stride) *out_stride = t.stride;
	if (cap_floats < need || (!out && need)) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu floats", need);
	if (int rc = read_now(ctx, out, (const float*)ps->d_channels.p + t.channel_base, need)) return rc;
	if (t.ribbon_len && out) { // the reference's layout: ribbon r's ring at [r x max_len, (r + 1) x max_len); the rings no ribbon holds behind them
		const LmxParticles::Emitter& em = ps->emitters[e];
		std::vector<float> row(t.capacity);
		for (uint32_t c = 0; c < t.channels; ++c) {
			float* o = out + (size_t)c * t.stride;
			memcpy(row.data(), o, (size_t)t.capacity * sizeof(float));
			uint32_t at = 0;
			for (const LmxParticles::Emitter::Ribbon& rb : em.ribbons) memcpy(o + (size_t)at++ * t.ribbon_len, row.data() + (size_t)rb.ring * t.ribbon_len, t.ribbon_len * sizeof(float));
			for (size_t k = em.free_rings.size(); k-- > 0;) memcpy(o + (size_t)at++ * t.ribbon_len, row.data() + (size_t)em.free_rings[k] * t.ribbon_len, t.ribbon_len * sizeof(float));
		}
	}
	return LMX_OK;
}

int lmx_particles_read_slices(LmxParticles* ps, LmxParticleSlice* slices, uint32_t cap_slices, void* data, uint32_t cap_bytes) {
	LMX_CHECK_PARTICLES(ps);
	if (int rc = build(ps)) return rc;
	if (cap_slices < ps->emitters.size() || (!slices && !ps->emitters.empty())) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu slices", ps->emitters.size());
	const size_t bytes = ((size_t)ps->frame_floats + PARTICLE_GUARD_FLOATS) * 4;
	if (data && cap_bytes < bytes) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu bytes", bytes);
	LMX_HIP(ctx, read_back(slices, (const LmxParticleSlice*)ps->d_slices.p, ps->emitters.size(), ctx->stream));
	return read_now(ctx, (float*)data, (const float*)ps->d_frame.p, bytes / 4);
}

int lmx_particles_set_emitter_options(LmxParticles* ps, uint32_t system, uint32_t emitter, const LmxParticleEmitterOptions* o) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (!o) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null options");
	if (!(o->emit_move_distance == o->emit_move_distance)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "emit_move_distance is not a number");
	LmxParticles::Emitter& em = ps->emitters[e];
	uint32_t len = 0;
	if (o->max_ribbons) {
		if (o->max_ribbon_length > PARTICLE_CHUNK)
			return fail(ctx, LMX_ERR_UNSUPPORTED, "max_ribbon_length %u: past 1024 the reference's chunk loop leaves its register pages and updates slots twice", o->max_ribbon_length);
		len = (o->max_ribbon_length + 3u) & ~3u; // as the resource loader does
		if (!len) return fail(ctx, LMX_ERR_INVALID, "a ribbon emitter with max_ribbon_length 0");
		if ((uint64_t)o->max_ribbons * len > MAX_CAPACITY) return fail(ctx, LMX_ERR_INVALID, "%u ribbons of %u points: at most 2^26 slots per emitter", o->max_ribbons, len);
		if (em.has_program)
			if (int rc = check_ribbon_program(ctx, em.prog)) return rc;
	}
	const bool was_ribbon = em.is_ribbon();
	em.opts = *o;
	em.ribbon_len = len;
	if (o->max_ribbons) em.capacity = o->max_ribbons * len;
	else if (was_ribbon) em.capacity = 0;
	em.ribbons.clear();
	em.free_rings.clear();
	ps->dirty = true;
	return LMX_OK;
}

int lmx_particles_emit_ribbons(LmxParticles* ps, uint32_t system, uint32_t emitter, uint32_t n) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (int rc = build(ps)) return rc;
	if (!ps->emitters[e].is_ribbon()) return LMX_OK; // (emitRibbons clamps to max_ribbons = 0)
	if (int rc = sync_sources(ps)) return rc;
	uint32_t set, lanes = 0;
	if (int rc = begin_upload(ps, &set)) return rc;
	const LmxParticles::System& sy = ps->systems[system];
	ParticleSystemDev& sv = ps->sys_host[system]; // TOTAL_TIME and TIME_DELTA are what the last step left; the entity is where it is now
	sv.values[PSV_ENTITY_X] = (float)sy.pos[0]; sv.values[PSV_ENTITY_Y] = (float)sy.pos[1]; sv.values[PSV_ENTITY_Z] = (float)sy.pos[2];
	std::vector<ParticleRibbonJob>& jobs = ps->rjobs_first_up[set];
	emit_ribbons_host(ps, e, n, sv.values[PSV_TOTAL_TIME], jobs, lanes);
	ps->sys_up[set] = ps->sys_host;
	LMX_HIP(ctx, upload_on_stream(ps->d_systems, ps->sys_up[set], ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_rjobs_first, jobs, ctx->stream));
	if (int rc = upload_ribbons(ps, set)) return rc;
	if (int rc = end_upload(ps, set)) return rc;
	LMX_HIP(ctx, launch_particles_ribbon_emit(ctx->stream, ps->dev(), ps->d_rjobs_first.p, (uint32_t)jobs.size(), lanes));
	return LMX_OK;
}

int lmx_particles_kill_ribbon(LmxParticles* ps, uint32_t system, uint32_t emitter, uint32_t ribbon) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	if (int rc = build(ps)) return rc;
	LmxParticles::Emitter& em = ps->emitters[e];
	if (ribbon >= em.ribbons.size()) return LMX_OK;
	// the ring map: the ribbons above move down one index and keep their rings, no byte moves (the reference's memmove, :1583-1591)
	em.free_rings.push_back(em.ribbons[ribbon].ring);
	em.ribbons.erase(em.ribbons.begin() + ribbon);
	ps->ribbons_changed = true;
	uint32_t set;
	if (int rc = begin_upload(ps, &set)) return rc;
	if (int rc = upload_ribbons(ps, set)) return rc;
	return end_upload(ps, set);
}

int lmx_particles_apply_transforms(LmxParticles* ps, uint32_t n_systems, const double* pos_xyz) {
	LMX_CHECK_PARTICLES(ps);
	if (n_systems != ps->systems.size() || (n_systems && !pos_xyz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%zu particle systems registered", ps->systems.size());
	if (int rc = build(ps)) return rc;
	if (ps->emitters.empty()) return LMX_OK;
	if (int rc = sync_sources(ps)) return rc;
	uint32_t set, lanes = 0, max_count = 0;
	if (int rc = begin_upload(ps, &set)) return rc;
	std::vector<ParticleEmitJob>& jobs = ps->jobs_first_up[set];
	std::vector<ParticleRibbonJob>& rjobs = ps->rjobs_first_up[set];
	for (uint32_t s = 0; s < n_systems; ++s) { // ParticleSystem::applyTransform (:1377-1403); of the transform only the position is used
		LmxParticles::System& sy = ps->systems[s];
		const double* np = pos_xyz + 3 * (size_t)s;
		memcpy(sy.pos, np, sizeof(double) * 3);
		ParticleSystemDev& sv = ps->sys_host[s];
		sv.values[PSV_ENTITY_X] = (float)np[0]; sv.values[PSV_ENTITY_Y] = (float)np[1]; sv.values[PSV_ENTITY_Z] = (float)np[2];
		sv.values[PSV_TOTAL_TIME] = sy.total_time;
		for (uint32_t e = sy.first; e < sy.first + sy.n; ++e) {
			LmxParticles::Emitter& em = ps->emitters[e];
			const float dist = em.opts.emit_move_distance;
			if (!(dist > 0)) continue;
			const double dx = np[0] - em.last_emit_point[0], dy = np[1] - em.last_emit_point[1], dz = np[2] - em.last_emit_point[2];
			if (!(dx * dx + dy * dy + dz * dz > (double)dist)) continue; // a squared length against an unsquared distance, as the reference compares
			memcpy(em.last_emit_point, np, sizeof(double) * 3);
			if (em.is_ribbon()) {
				for (uint32_t r = 0; r < em.ribbons.size(); ++r) emit_points_host(ps, e, r, 1, sy.total_time, 0.0f, rjobs, lanes);
			} else {
				jobs.push_back(ParticleEmitJob{e, 1, sy.total_time, 0.0f});
				max_count = 1;
			}
		}
	}
	ps->sys_up[set] = ps->sys_host;
	LMX_HIP(ctx, upload_on_stream(ps->d_systems, ps->sys_up[set], ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_jobs_first, jobs, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ps->d_rjobs_first, rjobs, ctx->stream));
	if (int rc = upload_ribbons(ps, set)) return rc;
	if (int rc = end_upload(ps, set)) return rc;
	const ParticlesDevice d = ps->dev();
	LMX_HIP(ctx, launch_particles_emit(ctx->stream, d, ps->d_jobs_first.p, (uint32_t)jobs.size(), max_count));
	LMX_HIP(ctx, launch_particles_ribbon_emit(ctx->stream, d, ps->d_rjobs_first.p, (uint32_t)rjobs.size(), lanes));
	return LMX_OK;
}

int lmx_particles_ribbons(LmxParticles* ps, uint32_t system, uint32_t emitter, LmxParticleRibbon* out, uint32_t cap, uint32_t* n) {
	LMX_CHECK_PARTICLES(ps);
	uint32_t e;
	if (int rc = find_emitter(ps, system, emitter, &e)) return rc;
	const LmxParticles::Emitter& em = ps->emitters[e];
	const uint32_t count = ps->dirty ? 0u : (uint32_t)em.ribbons.size(); // (a layout that is not built yet has no ribbons)
	if (n) *n = count;
	if (cap < count || (!out && count)) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u ribbons", count);
	uint32_t row = 0;
	for (uint32_t r = 0; r < count; ++r) {
		out[r] = LmxParticleRibbon{em.ribbons[r].offset, em.ribbons[r].length, em.ribbons[r].emit_index, row * em.outputs * 4u};
		row += em.ribbons[r].length;
	}
	return LMX_OK;
}

int lmx_particles_add_mesh(LmxParticles* ps, uint32_t n_verts, const float* positions_xyz, const LmxSkin* skin, uint32_t* out_mesh) {
	LMX_CHECK_PARTICLES(ps);
	if (!n_verts || !positions_xyz) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "a mesh needs at least one vertex");
	if (ps->mesh_positions.size() / 3 + (uint64_t)n_verts > (1u << 27)) return fail(ctx, LMX_ERR_CAPACITY, "more than 2^27 mesh vertices"); // (the kernels address both tables with 32-bit byte offsets)
	LmxParticles::Mesh m;
	m.vert_at = (uint32_t)(ps->mesh_positions.size() / 3);
	m.n_verts = n_verts;
	m.skin_at = skin ? (uint32_t)ps->mesh_skins.size() : PARTICLE_NO_SOURCE;
	ps->mesh_positions.insert(ps->mesh_positions.end(), positions_xyz, positions_xyz + 3 * (size_t)n_verts);
	if (skin) ps->mesh_skins.insert(ps->mesh_skins.end(), skin, skin + n_verts);
	if (out_mesh) *out_mesh = (uint32_t)ps->meshes.size();
	ps->meshes.push_back(m);
	ps->meshes_changed = true;
	return LMX_OK;
}

int lmx_particles_clear_meshes(LmxParticles* ps) {
	LMX_CHECK_PARTICLES(ps);
	ps->meshes.clear();
	ps->mesh_positions.clear();
	ps->mesh_skins.clear();
	for (LmxParticles::System& sy : ps->systems) sy.source.mesh = PARTICLE_NO_SOURCE; // a source that named a mesh has none until it is set again
	ps->meshes_changed = true;
	return LMX_OK;
}

int lmx_particles_set_mesh_source(LmxParticles* ps, uint32_t system, const LmxParticleMeshSource* source) {
	LMX_CHECK_PARTICLES(ps);
	if (system >= ps->systems.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "particle system %u: %zu registered", system, ps->systems.size());
	if (!source) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null mesh source");
	if (source->flags & ~(uint32_t)LMX_PARTICLE_MESH_HAS_BONES) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "mesh source flags %#x", source->flags);
	if (source->mesh != PARTICLE_NO_SOURCE) {
		if (source->mesh >= ps->meshes.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "mesh %u: %zu added", source->mesh, ps->meshes.size());
		if ((source->flags & LMX_PARTICLE_MESH_HAS_BONES) && ps->meshes[source->mesh].skin_at == PARTICLE_NO_SOURCE)
			return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the model has bones and mesh %u carries no skin", source->mesh);
	}
	LmxParticles::System& sy = ps->systems[system];
	sy.source = *source;
	sy.mesh_declared = true;
	ps->any_source = true;
	return LMX_OK;
}

int lmx_particles_set_spline(LmxParticles* ps, uint32_t system, const float* points_xyz, uint32_t n_points) {
	LMX_CHECK_PARTICLES(ps);
	if (system >= ps->systems.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "particle system %u: %zu registered", system, ps->systems.size());
	if (n_points == 1 || n_points == 2) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "a spline of %u points: the reference reads outside its array", n_points);
	if (n_points && !points_xyz) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null spline points");
	if (n_points > (1u << 24)) return fail(ctx, LMX_ERR_CAPACITY, "a spline of more than 2^24 points");
	LmxParticles::System& sy = ps->systems[system];
	sy.spline.assign(points_xyz, points_xyz + 3 * (size_t)n_points);
	sy.spline_declared = true;
	ps->splines_changed = true;
	ps->any_source = true;
	return LMX_OK;
}

int lmx_particles_device_outputs(LmxParticles* ps, LmxParticlesDevice* out) {
	LMX_CHECK_PARTICLES(ps);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (int rc = build(ps)) return rc;
	out->d_frame = ps->d_frame.p;
	out->d_slices = ps->d_slices.p;
	out->d_counts = (const LmxParticlesCounts*)ps->d_state.p;
	out->n_emitters = (uint32_t)ps->emitters.size();
	out->frame_bytes = ps->frame_floats * 4;
	return LMX_OK;
}

} // extern "C"
