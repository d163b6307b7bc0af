// lmx_capi_probes.hip — the probe bake's entry points (include/lumix_mi355.h, "Probe bake"): what EnvironmentProbePlugin
// (renderer/editor/render_plugins.cpp:3513-3870) does between "the six faces are captured" and "coefficients in the probe / RGBM bytes for the compressor", as an object
// beside the context. The host side validates the batch and launches probe_kernels.hip; the arithmetic is lmx_probes.h's.
#include "lmx_context.h"
#include "lmx_probes.h"

#include <cmath>

using namespace lmx;

struct LmxProbeBaker {
	LmxContext* ctx = nullptr;
	uint32_t n = 0, size = 0; // the batch of lmx_probes_set_cubemaps
	uint32_t table_size = 0;  // the S d_sh_table was built for; 0: none
	bool has_sh = false, has_mips = false, has_filtered = false, has_ggx = false;
	DevBuf<float> d_rgba, d_sh_table, d_sh, d_mips, d_ggx, d_filtered, d_dirs, d_lods, d_sampled;
	DevBuf<uint8_t> d_rgbm;
};

namespace {

// the first channel of `n` floats that is not finite, or n
size_t first_non_finite(const float* p, size_t n) {
	for (size_t i = 0; i < n; ++i)
		if (!std::isfinite(p[i])) return i;
	return n;
}

size_t mip_floats(const LmxProbeBaker* pb) { return 4 * (size_t)probe_mip_offset(pb->size, probe_log2(pb->size) + 1) * pb->n; }

int run_mips(LmxProbeBaker* pb) {
	LmxContext* ctx = pb->ctx;
	if (!probe_is_pow2(pb->size) || pb->size < 16) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: a reflection probe's size is a power of two of 16 or more, not %u", pb->size);
	if (pb->n > 65535) return fail(ctx, LMX_ERR_CAPACITY, "probes: %u reflection probes in one batch (65535 at most)", pb->n);
	if (int rc = Grow{ctx}(pb->d_mips, mip_floats(pb))) return rc;
	LMX_HIP(ctx, launch_probe_mips(ctx->stream, pb->d_rgba.p, pb->n, pb->size, pb->d_mips.p));
	pb->has_mips = true;
	return LMX_OK;
}

ProbeChain chain_of(const LmxProbeBaker* pb) { return ProbeChain{pb->d_rgba.p, pb->d_mips.p, pb->n, pb->size, probe_log2(pb->size)}; }

size_t filtered_texels(const LmxProbeBaker* pb) { return (size_t)probe_level_offset(pb->size, GGX_LEVELS) * pb->n; }

} // namespace

extern "C" {

int lmx_probes_ggx_samples(uint32_t level, float* out) {
	if (!out || level >= GGX_LEVELS) return LMX_ERR_INVALID_ARGUMENT;
	const float roughness = (float)level / (float)(GGX_LEVELS - 1);
	for (uint32_t i = 0; i < GGX_SAMPLES; ++i) {
		const V3 h = ggx_sample_h(i, roughness);
		out[3 * i] = h.x;
		out[3 * i + 1] = h.y;
		out[3 * i + 2] = h.z;
	}
	return LMX_OK;
}

int lmx_probes_batch_bytes(uint32_t n, uint32_t size, uint64_t* out) {
	if (!out) return LMX_ERR_INVALID_ARGUMENT;
	*out = 0;
	if (n == 0 || size == 0) return LMX_ERR_INVALID_ARGUMENT;
	const uint64_t bytes = probe_batch_bytes(n, size);
	if (bytes == 0) return LMX_ERR_CAPACITY;
	*out = bytes;
	return LMX_OK;
}

int lmx_probes_create(LmxContext* ctx, LmxProbeBaker** out) { return object_create(ctx, out, "probes"); }

void lmx_probes_destroy(LmxProbeBaker* pb) {
	if (pb) object_destroy(pb);
}

int lmx_probes_set_cubemaps(LmxProbeBaker* pb, uint32_t n, uint32_t size, const float* rgba) {
	LMX_ENTER(pb);
	if (n == 0 || size == 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: a batch of %u cubemaps of size %u", n, size);
	const uint64_t bytes = probe_batch_bytes(n, size);
	if (bytes == 0) return fail(ctx, LMX_ERR_CAPACITY, "probes: %u cubemaps of size %u are above the batch cap of %llu bytes", n, size, (unsigned long long)PROBES_MAX_BATCH_BYTES);
	if (!rgba) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: null cubemaps");
	const size_t floats = (size_t)(bytes / 4);
	const size_t bad = first_non_finite(rgba, floats);
	if (bad != floats) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: channel %zu of texel %zu is not finite", bad % 4, bad / 4);
	if (int rc = upload_settled(ctx, pb->d_rgba, rgba, floats)) return rc;
	pb->n = n;
	pb->size = size;
	pb->has_sh = pb->has_mips = pb->has_filtered = false;
	return LMX_OK;
}

int lmx_probes_sh_run(LmxProbeBaker* pb) {
	LMX_ENTER(pb);
	if (!pb->n) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: sh_run before set_cubemaps");
	if (pb->table_size != pb->size) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a queued kernel may still read the table a reserve frees)
		pb->table_size = 0;
		LMX_HIP(ctx, pb->d_sh_table.reserve((size_t)SH_TABLE_ROWS * probe_texels(pb->size)));
		LMX_HIP(ctx, launch_sh_table(ctx->stream, pb->size, pb->d_sh_table.p));
		pb->table_size = pb->size;
	}
	if (int rc = Grow{ctx}(pb->d_sh, 27 * (size_t)pb->n)) return rc; // (behind the table's launch: a Grow of its own)
	LMX_HIP(ctx, launch_sh_accumulate(ctx->stream, pb->d_rgba.p, pb->d_sh_table.p, pb->n, pb->size, pb->d_sh.p));
	pb->has_sh = true;
	return LMX_OK;
}

int lmx_probes_read_sh(LmxProbeBaker* pb, float* out, uint32_t cap_probes) {
	LMX_ENTER(pb);
	if (!pb->has_sh) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: no sh_run on this batch");
	return read_out(ctx, out, 27 * (size_t)cap_probes, (const float*)pb->d_sh.p, 27 * (size_t)pb->n, 27 * (size_t)pb->n, "floats of SH (27 per probe)", NullOut::Refused);
}

int lmx_probes_mips_run(LmxProbeBaker* pb) {
	LMX_ENTER(pb);
	if (!pb->n) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: mips_run before set_cubemaps");
	return run_mips(pb);
}

int lmx_probes_filter_run(LmxProbeBaker* pb) {
	LMX_ENTER(pb);
	if (!pb->n) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: filter_run before set_cubemaps");
	if (int rc = run_mips(pb)) return rc;
	if (!pb->has_ggx) {
		std::vector<float> table((size_t)GGX_LEVELS * GGX_SAMPLES * 3);
		for (uint32_t level = 0; level < GGX_LEVELS; ++level) lmx_probes_ggx_samples(level, table.data() + (size_t)level * GGX_SAMPLES * 3);
		if (int rc = upload_settled(ctx, pb->d_ggx, table.data(), table.size())) return rc;
		pb->has_ggx = true;
	}
	const size_t texels = filtered_texels(pb);
	Grow grow{ctx};
	if (int rc = grow(pb->d_filtered, 4 * texels)) return rc;
	if (int rc = grow(pb->d_rgbm, 4 * texels)) return rc;
	LMX_HIP(ctx, launch_probe_filter(ctx->stream, chain_of(pb), pb->d_ggx.p, pb->d_filtered.p));
	LMX_HIP(ctx, launch_probe_rgbm(ctx->stream, pb->d_filtered.p, pb->n, pb->size, pb->d_rgbm.p));
	pb->has_filtered = true;
	return LMX_OK;
}

int lmx_probes_sample(LmxProbeBaker* pb, uint32_t probe, uint32_t n, const float* dirs, const float* lods, float* out) {
	LMX_ENTER(pb);
	if (!pb->has_mips) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: sample before mips_run / filter_run");
	if (probe >= pb->n) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: probe %u of %u", probe, pb->n);
	if (!n) return LMX_OK;
	if (!dirs || !lods || !out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: null directions / lods / output");
	for (uint32_t i = 0; i < n; ++i) {
		const float* d = dirs + 3 * (size_t)i;
		if (first_non_finite(d, 3) != 3 || !std::isfinite(lods[i])) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: direction or lod %u is not finite", i);
		if (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "probes: direction %u is zero", i);
	}
	if (int rc = upload_settled(ctx, pb->d_dirs, dirs, 3 * (size_t)n)) return rc;
	if (int rc = upload_settled(ctx, pb->d_lods, lods, (size_t)n)) return rc;
	// (the stream has drained: nothing reads the buffer a reserve frees)
	LMX_HIP(ctx, pb->d_sampled.reserve(3 * (size_t)n));
	LMX_HIP(ctx, launch_probe_sample(ctx->stream, chain_of(pb), probe, pb->d_dirs.p, pb->d_lods.p, n, pb->d_sampled.p));
	return read_now(ctx, out, (const float*)pb->d_sampled.p, 3 * (size_t)n);
}

int lmx_probes_read_mips(LmxProbeBaker* pb, float* out, uint64_t cap_floats) {
	LMX_ENTER(pb);
	if (!pb->has_mips) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: no mips_run on this batch");
	return read_out(ctx, out, (size_t)cap_floats, (const float*)pb->d_mips.p, mip_floats(pb), mip_floats(pb), "floats of mips", NullOut::Refused);
}

int lmx_probes_read_filtered(LmxProbeBaker* pb, float* out, uint64_t cap_floats) {
	LMX_ENTER(pb);
	if (!pb->has_filtered) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: no filter_run on this batch");
	const size_t floats = 4 * filtered_texels(pb);
	return read_out(ctx, out, (size_t)cap_floats, (const float*)pb->d_filtered.p, floats, floats, "filtered floats", NullOut::Refused);
}

int lmx_probes_read_rgbm(LmxProbeBaker* pb, uint8_t* out, uint64_t cap_bytes) {
	LMX_ENTER(pb);
	if (!pb->has_filtered) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: no filter_run on this batch");
	const size_t bytes = 4 * filtered_texels(pb);
	return read_out(ctx, out, (size_t)cap_bytes, (const uint8_t*)pb->d_rgbm.p, bytes, bytes, "RGBM bytes", NullOut::Refused);
}

int lmx_probes_device_outputs(LmxProbeBaker* pb, LmxProbesDevice* out) {
	LMX_ENTER(pb);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!pb->n) return fail(ctx, LMX_ERR_NOT_BUILT, "probes: no cubemaps");
	out->d_cubemaps = pb->d_rgba.p;
	out->d_sh = pb->has_sh ? pb->d_sh.p : nullptr;
	out->d_mips = pb->has_mips ? pb->d_mips.p : nullptr;
	out->d_filtered = pb->has_filtered ? pb->d_filtered.p : nullptr;
	out->d_rgbm = pb->has_filtered ? pb->d_rgbm.p : nullptr;
	out->n = pb->n;
	out->size = pb->size;
	return LMX_OK;
}

} // extern "C"
