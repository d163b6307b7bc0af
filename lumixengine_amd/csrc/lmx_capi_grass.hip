// lmx_capi_grass.hip — terrain grass entry points (include/lumix_mi355.h, "Terrain grass"): the terrain table, the bookkeeping of
// Terrain::createGrass (renderer/terrain.cpp:26-139) in plain C++ on the host - which quads exist, last_used_frame, the eviction with its
// u32 wrap, the loop bounds with their truncations - the launch of every new quad of a frame (grass_kernels.hip), and renderGrass's quad
// loop (renderer/pipeline.cpp:2119-2209) for every view of a frame. lmx_grass_update and lmx_grass_cull do not wait for the device.
#include "lmx_context.h"
#include "lmx_grass.h"

#include <cmath>
#include <map>

using namespace lmx;

namespace {

static_assert(sizeof(LmxGrassType) == 16 && sizeof(LmxGrassTerrain) == 80 && sizeof(LmxGrassInstance) == 32 && sizeof(LmxGrassQuad) == 48, "table records");
static_assert(sizeof(LmxGrassView) == 288 && sizeof(LmxGrassDraw) == 24 && sizeof(LmxGrassCounts) == 16, "view records");

// A host array on its way to the device without a wait: two pinned halves take turns, each with the event recorded behind its copy. The
// half an upload reuses was copied two uploads ago; its event is waited for (it has long passed) before the host writes it again.
struct Staged {
	void* host[2] = {nullptr, nullptr};
	size_t cap[2] = {0, 0};
	hipEvent_t done[2] = {nullptr, nullptr};
	uint32_t next = 0;
	Staged() = default;
	Staged(const Staged&) = delete;
	Staged& operator=(const Staged&) = delete;
	~Staged() {
		for (int i = 0; i < 2; ++i) {
			if (host[i]) (void)hipHostFree(host[i]);
			if (done[i]) (void)hipEventDestroy(done[i]);
		}
	}
	// precondition: `dst` holds n elements
	template <typename T> hipError_t upload(T* dst, const T* src, size_t n, hipStream_t stream) {
		if (!n) return hipSuccess;
		const uint32_t h = next;
		const size_t bytes = n * sizeof(T);
		hipError_t e;
		if (!done[h]) {
			if ((e = hipEventCreateWithFlags(&done[h], hipEventDisableTiming)) != hipSuccess) return e;
		} else if ((e = hipEventSynchronize(done[h])) != hipSuccess) {
			return e;
		}
		if (cap[h] < bytes) {
			if (host[h]) (void)hipHostFree(host[h]);
			host[h] = nullptr;
			cap[h] = 0;
			if ((e = hipHostMalloc(&host[h], bytes + bytes / 4 + 256, hipHostMallocDefault)) != hipSuccess) return e;
			cap[h] = bytes + bytes / 4 + 256;
		}
		memcpy(host[h], src, bytes);
		if ((e = hipMemcpyAsync(dst, host[h], bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
		if ((e = hipEventRecord(done[h], stream)) != hipSuccess) return e;
		next ^= 1u;
		return hipSuccess;
	}
};

struct CachedQuad { uint32_t slot, last_used_frame; };

struct GrassTypeHost {
	LmxGrassType t = {};
	std::map<uint64_t, CachedQuad> quads; // key (u64(i) << 32) | j, :78: iterated in (i, j) order
};

struct GrassTerrainHost {
	bool height_ready = false, splat_ready = false;
	double pos[3] = {0, 0, 0};
	std::vector<GrassTypeHost> types;
};

} // namespace

struct LmxGrass {
	LmxContext* ctx = nullptr;
	std::vector<GrassTerrainHost> terrains;
	std::vector<GrassGroupDev> groups;     // (terrain, type) in table order
	std::vector<uint32_t> first_group;     // per terrain
	bool have_terrains = false;
	uint32_t n_slots = 0;
	std::vector<uint32_t> free_slots;      // popped from the back: lowest slot first
	std::vector<GrassLive> live;           // host copy of d_live
	std::vector<LmxGrassQuad> live_meta;   // ij / type / terrain / slot per live quad (the device holds the rest)
	bool live_dirty = true, pos_dirty = true;
	uint32_t n_views = 0, draw_stride = 0, cull_live = 0; // of the last cull
	bool culled = false;
	DevBuf<uint8_t> d_texels;
	DevBuf<GrassTerrainDev> d_terrains;
	DevBuf<GrassGroupDev> d_groups;
	DevBuf<double> d_pos;
	DevBuf<float4> d_pool;
	DevBuf<LmxGrassQuad> d_quads;
	DevBuf<GrassJob> d_jobs;
	DevBuf<GrassLive> d_live;
	DevBuf<GrassViewDev> d_views;
	DevBuf<LmxGrassDraw> d_draws;
	DevBuf<LmxGrassCounts> d_counts;
	Staged s_jobs, s_live, s_views, s_pos;
};

namespace {

void drop_terrain_quads(LmxGrass* g, uint32_t k) {
	for (GrassTypeHost& ty : g->terrains[k].types) {
		for (auto& kv : ty.quads) g->free_slots.push_back(kv.second.slot);
		if (!ty.quads.empty()) g->live_dirty = true;
		ty.quads.clear();
	}
}

void reset_slots(LmxGrass* g) {
	for (GrassTerrainHost& t : g->terrains)
		for (GrassTypeHost& ty : t.types) ty.quads.clear();
	g->free_slots.resize(g->n_slots);
	for (uint32_t s = 0; s < g->n_slots; ++s) g->free_slots[s] = g->n_slots - 1 - s;
	g->live_dirty = true;
}

// a slot freed and taken again within one update keeps the order "lowest free slot first"
void sort_free(LmxGrass* g) { std::sort(g->free_slots.begin(), g->free_slots.end(), [](uint32_t a, uint32_t b) { return a > b; }); }

// (int)v of IVec2(Vec2) and u32(v) of the loop bounds are undefined outside their types: refused instead
bool int_ok(float v) { return std::isfinite(v) && v > -2147483648.0f && v < 2147483648.0f; }

void rebuild_live(LmxGrass* g) {
	g->live.clear();
	g->live_meta.clear();
	for (uint32_t k = 0; k < g->terrains.size(); ++k)
		for (uint32_t t = 0; t < g->terrains[k].types.size(); ++t)
			for (const auto& kv : g->terrains[k].types[t].quads) {
				g->live.push_back(GrassLive{kv.second.slot, g->first_group[k] + t});
				LmxGrassQuad m;
				memset(&m, 0, sizeof(m));
				m.ij[0] = (int32_t)(uint32_t)(kv.first >> 32); m.ij[1] = (int32_t)(uint32_t)kv.first;
				m.type = t; m.terrain = k; m.slot = kv.second.slot;
				g->live_meta.push_back(m);
			}
}

} // namespace

extern "C" {

int lmx_grass_create(LmxContext* ctx, LmxGrass** out) { return object_create(ctx, out, "grass"); }

void lmx_grass_destroy(LmxGrass* g) {
	if (g) object_destroy(g);
}

int lmx_grass_set_terrains(LmxGrass* g, uint32_t n, const LmxGrassTerrain* terrains) {
	LMX_ENTER(g);
	if (n && !terrains) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null terrain table");
	if (n > LMX_GRASS_MAX_TERRAINS) return fail(ctx, LMX_ERR_CAPACITY, "%u terrains: at most %d", n, LMX_GRASS_MAX_TERRAINS);
	std::vector<GrassTerrainDev> recs(n);
	std::vector<GrassTerrainHost> hosts(n);
	std::vector<GrassGroupDev> groups;
	std::vector<uint32_t> first_group(n);
	uint64_t bytes = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const LmxGrassTerrain& in = terrains[k];
		const LmxRayTerrain& hm = in.heightmap;
		if (hm.format != LMX_RAY_TERRAIN_R16 && hm.format != LMX_RAY_TERRAIN_RGBA8) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: heightmap format %u", k, hm.format);
		if (hm.ready && (!hm.texels || hm.width == 0 || hm.height == 0)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: ready without a %u x %u heightmap", k, hm.width, hm.height);
		if (hm.ready && (uint64_t)hm.width * hm.height > (1ull << 30)) return fail(ctx, LMX_ERR_CAPACITY, "terrain %u: %u x %u texels: at most 2^30", k, hm.width, hm.height);
		if (in.n_types > LMX_GRASS_MAX_TYPES) return fail(ctx, LMX_ERR_CAPACITY, "terrain %u: %u grass types: at most %d", k, in.n_types, LMX_GRASS_MAX_TYPES);
		if (in.n_types && !in.types) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: null grass types", k);
		const bool splat_ok = in.splat_ready && in.splat_format == LMX_RAY_TERRAIN_RGBA8 && in.splat_texels && in.splat_width && in.splat_height;
		if (splat_ok && (uint64_t)in.splat_width * in.splat_height > (1ull << 30)) return fail(ctx, LMX_ERR_CAPACITY, "terrain %u: %u x %u splat texels: at most 2^30", k, in.splat_width, in.splat_height);
		for (uint32_t t = 0; t < in.n_types; ++t)
			if (in.types[t].rotation_mode != LMX_GRASS_ROTATION_Y_UP && in.types[t].rotation_mode != LMX_GRASS_ROTATION_ALL_RANDOM)
				return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u type %u: rotation mode %u", k, t, in.types[t].rotation_mode);
		GrassTerrainDev& r = recs[k];
		memset(&r, 0, sizeof(r));
		r.width = hm.width; r.height = hm.height; r.format = hm.format;
		for (int c = 0; c < 3; ++c) r.scale[c] = hm.scale[c];
		r.height_at = bytes;
		if (hm.ready) bytes += ((uint64_t)hm.width * hm.height * (hm.format == LMX_RAY_TERRAIN_R16 ? 2 : 4) + 3) & ~3ull;
		r.splat_at = bytes;
		r.splat_w = in.splat_width; r.splat_h = in.splat_height; r.splat_ok = splat_ok ? 1u : 0u;
		if (splat_ok) bytes += (uint64_t)in.splat_width * in.splat_height * 4;
		GrassTerrainHost& h = hosts[k];
		h.height_ready = hm.ready != 0;
		h.splat_ready = in.splat_ready != 0;
		h.types.resize(in.n_types);
		first_group[k] = (uint32_t)groups.size();
		for (uint32_t t = 0; t < in.n_types; ++t) {
			h.types[t].t = in.types[t];
			groups.push_back(GrassGroupDev{k, t, in.types[t].spacing, in.types[t].distance, in.types[t].usable ? 1u : 0u, 0u});
		}
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, g->d_texels.reserve(std::max<size_t>((size_t)bytes, 4)));
	for (uint32_t k = 0; k < n; ++k) {
		const LmxGrassTerrain& in = terrains[k];
		if (in.heightmap.ready)
			LMX_HIP(ctx, upload_blocking(g->d_texels.p + recs[k].height_at, (const uint8_t*)in.heightmap.texels, (size_t)in.heightmap.width * in.heightmap.height * (in.heightmap.format == LMX_RAY_TERRAIN_R16 ? 2 : 4)));
		if (recs[k].splat_ok) LMX_HIP(ctx, upload_blocking(g->d_texels.p + recs[k].splat_at, (const uint8_t*)in.splat_texels, (size_t)in.splat_width * in.splat_height * 4));
	}
	LMX_HIP(ctx, upload_blocking(g->d_terrains, recs));
	LMX_HIP(ctx, upload_blocking(g->d_groups, groups));
	LMX_HIP(ctx, g->d_pos.reserve(std::max<size_t>(3 * (size_t)n, 3)));
	g->terrains.swap(hosts);
	g->groups.swap(groups);
	g->first_group.swap(first_group);
	g->have_terrains = true;
	g->culled = false;
	g->pos_dirty = true;
	reset_slots(g); // m_is_grass_dirty of every terrain
	return LMX_OK;
}

int lmx_grass_invalidate(LmxGrass* g, uint32_t terrain) {
	LMX_ENTER(g);
	if (terrain != 0xffffffffu && terrain >= g->terrains.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown terrain %u (%zu set)", terrain, g->terrains.size());
	for (uint32_t k = 0; k < g->terrains.size(); ++k)
		if (terrain == 0xffffffffu || terrain == k) drop_terrain_quads(g, k);
	sort_free(g);
	return LMX_OK;
}

int lmx_grass_set_positions(LmxGrass* g, uint32_t n, const double* pos_xyz) {
	LMX_ENTER(g);
	if (n > g->terrains.size() || (n && !pos_xyz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%u positions for %zu terrains", n, g->terrains.size());
	for (uint32_t k = 0; k < n; ++k)
		for (int c = 0; c < 3; ++c) g->terrains[k].pos[c] = pos_xyz[3 * (size_t)k + c];
	g->pos_dirty = true;
	return LMX_OK;
}

int lmx_grass_reserve(LmxGrass* g, uint32_t slots) {
	LMX_ENTER(g);
	if (slots > (1u << 20)) return fail(ctx, LMX_ERR_CAPACITY, "%u slots: at most 2^20 (64 GiB of instances)", slots);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, g->d_pool.reserve(std::max<size_t>((size_t)slots * 2 * LMX_GRASS_SLOT_INSTANCES, 1)));
	LMX_HIP(ctx, g->d_quads.reserve(std::max<size_t>(slots, 1)));
	g->n_slots = slots;
	g->culled = false;
	reset_slots(g);
	return LMX_OK;
}

int lmx_grass_update(LmxGrass* g, uint32_t frame, uint32_t n, const float* center_xz) {
	LMX_ENTER(g);
	if (!g->have_terrains) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_grass_set_terrains has not been called");
	if (n != g->terrains.size() || (n && !center_xz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "%u centres for %zu terrains", n, g->terrains.size());
	// 1. what the call would do, without doing it: the quads it evicts, touches and creates
	struct Plan { int32_t i0 = 0, j0 = 0; uint32_t cols = 0, rows = 0; bool run = false; };
	std::vector<std::vector<Plan>> plans(n);
	uint64_t freed = 0, needed = 0;
	for (uint32_t k = 0; k < n; ++k) {
		const GrassTerrainHost& te = g->terrains[k];
		plans[k].resize(te.types.size());
		if (!te.height_ready || !te.splat_ready) continue; // :38-41
		const float cx = center_xz[2 * (size_t)k], cz = center_xz[2 * (size_t)k + 1];
		if (!std::isfinite(cx) || !std::isfinite(cz)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u: centre (%g, %g)", k, cx, cz);
		for (uint32_t t = 0; t < te.types.size(); ++t) {
			const GrassTypeHost& ty = te.types[t];
			for (const auto& kv : ty.quads)
				if (kv.second.last_used_frame < frame - 3u) ++freed; // :46: u32, wraps for frame < 3
			if (ty.t.spacing <= 0) continue; // :56
			Plan& p = plans[k][t];
			const float quad_size = ty.t.spacing * 32; // :61
			const float qx = (cx - ty.t.distance) / quad_size, qz = (cz - ty.t.distance) / quad_size; // (center - half_extents) / quad_size, :62
			const float span = (ty.t.distance * 2) / quad_size; // size.x / quad_size.x, :72
			if (!int_ok(qx) || !int_ok(qz) || !int_ok(span) || span < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u type %u: quad indices (%g, %g) + %g outside int", k, t, qx, qz, span);
			p.i0 = std::max((int32_t)qx, 0); p.j0 = std::max((int32_t)qz, 0); // maximum(IVec2(...), IVec2(0))
			p.cols = p.rows = 1u + (uint32_t)span;
			if ((uint64_t)(uint32_t)p.i0 + p.cols > 0x7fffffffull || (uint64_t)(uint32_t)p.j0 + p.rows > 0x7fffffffull)
				return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "terrain %u type %u: quad indices past int", k, t);
			p.run = true;
			if ((uint64_t)p.cols * p.rows > (uint64_t)g->n_slots) return fail(ctx, LMX_ERR_CAPACITY, "terrain %u type %u: %u x %u quads in range, %u slots reserved", k, t, p.cols, p.rows, g->n_slots);
			for (uint32_t j = (uint32_t)p.j0; j < (uint32_t)p.j0 + p.rows; ++j)
				for (uint32_t i = (uint32_t)p.i0; i < (uint32_t)p.i0 + p.cols; ++i) {
					const auto it = ty.quads.find(((uint64_t)i << 32) | j);
					if (it == ty.quads.end() || it->second.last_used_frame < frame - 3u) ++needed; // (an evicted quad in range is created again)
				}
		}
	}
	if (needed > g->free_slots.size() + freed)
		return fail(ctx, LMX_ERR_CAPACITY, "the update creates %llu quads: %zu slots free and %llu freed by it, of %u", (unsigned long long)needed, g->free_slots.size(), (unsigned long long)freed, g->n_slots);
	// 2. the same, for real: evict, then touch or create in the reference's order (type by type, rows of j, i within)
	std::vector<GrassJob> jobs;
	for (uint32_t k = 0; k < n; ++k) {
		GrassTerrainHost& te = g->terrains[k];
		if (!te.height_ready || !te.splat_ready) continue;
		for (GrassTypeHost& ty : te.types)
			for (auto it = ty.quads.begin(); it != ty.quads.end();) {
				if (it->second.last_used_frame < frame - 3u) {
					g->free_slots.push_back(it->second.slot);
					it = ty.quads.erase(it);
					g->live_dirty = true;
				} else ++it;
			}
	}
	sort_free(g);
	for (uint32_t k = 0; k < n; ++k) {
		GrassTerrainHost& te = g->terrains[k];
		for (uint32_t t = 0; t < plans[k].size(); ++t) {
			const Plan& p = plans[k][t];
			if (!p.run) continue;
			GrassTypeHost& ty = te.types[t];
			for (uint32_t j = (uint32_t)p.j0; j < (uint32_t)p.j0 + p.rows; ++j)
				for (uint32_t i = (uint32_t)p.i0; i < (uint32_t)p.i0 + p.cols; ++i) {
					const uint64_t key = ((uint64_t)i << 32) | j;
					const auto it = ty.quads.find(key);
					if (it != ty.quads.end()) {
						it->second.last_used_frame = frame; // :82
						continue;
					}
					const uint32_t slot = g->free_slots.back(); // (counted above: there is one)
					g->free_slots.pop_back();
					ty.quads.emplace(key, CachedQuad{slot, frame});
					jobs.push_back(GrassJob{k, t, i, j, slot, ty.t.rotation_mode, ty.t.spacing, 0u});
					g->live_dirty = true;
				}
		}
	}
	if (jobs.empty()) return LMX_OK;
	if (int rc = Grow{ctx}(g->d_jobs, jobs.size())) return rc;
	LMX_HIP(ctx, g->s_jobs.upload(g->d_jobs.p, jobs.data(), jobs.size(), ctx->stream));
	GrassQuadsDevice d;
	d.terrains = g->d_terrains.p; d.texels = g->d_texels.p; d.jobs = g->d_jobs.p; d.n_jobs = (uint32_t)jobs.size();
	d.pool = g->d_pool.p; d.quads = g->d_quads.p;
	LMX_HIP(ctx, launch_grass_quads(ctx->stream, d));
	return LMX_OK;
}

int lmx_grass_cull(LmxGrass* g, uint32_t n_views, const LmxGrassView* views) {
	LMX_ENTER(g);
	if (!n_views) return LMX_OK;
	if (!views) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null views");
	if (!g->have_terrains) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_grass_set_terrains has not been called");
	if (n_views > LMX_MAX_VIEWS) return fail(ctx, LMX_ERR_CAPACITY, "%u views: at most %d", n_views, LMX_MAX_VIEWS);
	if (g->live_dirty) {
		rebuild_live(g);
		if (int rc = Grow{ctx}(g->d_live, std::max<size_t>(g->live.size(), 1))) return rc;
		LMX_HIP(ctx, g->s_live.upload(g->d_live.p, g->live.data(), g->live.size(), ctx->stream));
		g->live_dirty = false;
	}
	if (g->pos_dirty) {
		std::vector<double> pos(3 * g->terrains.size());
		for (size_t k = 0; k < g->terrains.size(); ++k)
			for (int c = 0; c < 3; ++c) pos[3 * k + c] = g->terrains[k].pos[c];
		LMX_HIP(ctx, g->s_pos.upload(g->d_pos.p, pos.data(), pos.size(), ctx->stream));
		g->pos_dirty = false;
	}
	const uint32_t n_live = (uint32_t)g->live.size();
	const uint32_t stride = std::max<uint32_t>(n_live, 1);
	Grow grow{ctx}; // (behind the copies of the live list and the positions: a Grow of its own)
	if (int rc = grow(g->d_views, n_views)) return rc;
	if (int rc = grow(g->d_counts, n_views)) return rc;
	if (int rc = grow(g->d_draws, (size_t)n_views * stride)) return rc;
	std::vector<GrassViewDev> vd(n_views);
	for (uint32_t v = 0; v < n_views; ++v) {
		memset(&vd[v], 0, sizeof(GrassViewDev));
		vd[v].f = to_dev_frustum(views[v].frustum);
		for (int c = 0; c < 3; ++c) vd[v].viewport[c] = views[v].viewport_pos[c];
		vd[v].lod_multiplier = views[v].lod_multiplier;
	}
	LMX_HIP(ctx, g->s_views.upload(g->d_views.p, vd.data(), vd.size(), ctx->stream));
	GrassCullDevice d;
	d.views = g->d_views.p; d.live = g->d_live.p; d.n_live = n_live; d.draw_stride = stride;
	d.groups = g->d_groups.p; d.terrain_pos = g->d_pos.p; d.quads = g->d_quads.p;
	d.draws = g->d_draws.p; d.counts = g->d_counts.p;
	LMX_HIP(ctx, launch_grass_cull(ctx->stream, d, n_views));
	g->n_views = n_views;
	g->draw_stride = stride;
	g->cull_live = n_live;
	g->culled = true;
	return LMX_OK;
}

int lmx_grass_read_quads(LmxGrass* g, LmxGrassQuad* out, uint32_t cap, uint32_t* out_n) {
	LMX_ENTER(g);
	if (g->live_dirty) rebuild_live(g); // (the device list goes up with the next cull: live_dirty stays set)
	const uint32_t n = (uint32_t)g->live.size();
	if (out_n) *out_n = n;
	if (cap < n) return fail(ctx, LMX_ERR_CAPACITY, "%u live quads, cap %u", n, cap);
	if (!n) return LMX_OK;
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	std::vector<LmxGrassQuad> all(g->n_slots);
	if (int rc = read_now(ctx, all.data(), (const LmxGrassQuad*)g->d_quads.p, all.size())) return rc;
	for (uint32_t q = 0; q < n; ++q) out[q] = all[g->live[q].slot];
	return LMX_OK;
}

int lmx_grass_read_instances(LmxGrass* g, uint32_t slot, LmxGrassInstance* out, uint32_t cap) {
	LMX_ENTER(g);
	if (slot >= g->n_slots) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "slot %u of %u", slot, g->n_slots);
	return read_out(ctx, out, cap, (const LmxGrassInstance*)(g->d_pool.p + (size_t)slot * 2 * LMX_GRASS_SLOT_INSTANCES), LMX_GRASS_SLOT_INSTANCES, LMX_GRASS_SLOT_INSTANCES,
		"records of a slot", NullOut::Refused);
}

int lmx_grass_write_instances(LmxGrass* g, uint32_t slot, const LmxGrassInstance* in, uint32_t n) {
	LMX_ENTER(g);
	if (slot >= g->n_slots || n > LMX_GRASS_SLOT_INSTANCES) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "slot %u of %u, %u records", slot, g->n_slots, n);
	if (n && !in) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null records");
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking((LmxGrassInstance*)(g->d_pool.p + (size_t)slot * 2 * LMX_GRASS_SLOT_INSTANCES), in, n));
	return LMX_OK;
}

int lmx_grass_read_draws(LmxGrass* g, uint32_t view, LmxGrassDraw* out, uint32_t cap, uint32_t* out_n) {
	LMX_ENTER(g);
	if (!g->culled) return fail(ctx, LMX_ERR_NOT_BUILT, "no lmx_grass_cull has run");
	if (view >= g->n_views) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "view %u of %u", view, g->n_views);
	LmxGrassCounts c;
	if (int rc = read_now(ctx, &c, (const LmxGrassCounts*)g->d_counts.p + view, 1)) return rc;
	if (out_n) *out_n = c.draws;
	return read_out(ctx, out, cap, (const LmxGrassDraw*)g->d_draws.p + (size_t)view * g->draw_stride, c.draws, c.draws, "draws", NullOut::Refused);
}

int lmx_grass_counts(LmxGrass* g, LmxGrassCounts* out, uint32_t cap_views) {
	LMX_ENTER(g);
	if (!g->culled) return fail(ctx, LMX_ERR_NOT_BUILT, "no lmx_grass_cull has run");
	return read_out(ctx, out, cap_views, (const LmxGrassCounts*)g->d_counts.p, g->n_views, g->n_views, "views' counts", NullOut::Refused); // (a cull has at least one view)
}

int lmx_grass_device_outputs(LmxGrass* g, LmxGrassDevice* out) {
	LMX_ENTER(g);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!g->n_slots) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_grass_reserve has not been called");
	memset(out, 0, sizeof(*out));
	out->d_pool = (const LmxGrassInstance*)g->d_pool.p;
	out->d_quads = g->d_quads.p;
	out->n_slots = g->n_slots;
	if (g->culled) {
		out->d_draws = g->d_draws.p; out->d_counts = g->d_counts.p;
		out->draw_stride = g->draw_stride; out->n_views = g->n_views; out->n_live = g->cull_live;
	}
	return LMX_OK;
}

} // extern "C"
