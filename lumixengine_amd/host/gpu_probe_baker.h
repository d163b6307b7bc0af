// gpu_probe_baker.h — the probe bake's host adapter (C++ host side of include/lumix_mi355.h "Probe bake").
//
// In the reference EnvironmentProbePlugin (src/renderer/editor/render_plugins.cpp:3513-3870) captures six faces per probe into a ProbeJob
// and then, per job, either runs SphericalHarmonics::compute on the read-back capture (:3752) and copies the coefficients into the
// EnvironmentProbe when every job is done (:3854-3858), or builds the mip chain, filters five roughness levels and encodes them to RGBM
// for TextureCompressor (saveCubemap, :3535-3577). GpuProbeBaker takes the captures of a batch of jobs and does what lies between:
//   bakeEnvironment(jobs, probes, n)   SH of n captures of one size; probes[i]->sh_coefs written as :3858 does
//   bakeReflection(jobs, n)            mips, radiance levels and RGBM of n captures of one size (a power of two of 16 or more)
//   rgbm(job, face, level)             the bytes of one image, ready for `input.add(face, 0, level).pixels`
// The capture itself (Pipeline::render into the faces), TextureCompressor::compress and the file writes stay with the engine.
// Every member returns false where the library refuses (lastError() says why): the caller then runs the plugin's own path.
//
// `JobT` is ProbeJob-shaped: `data` with begin() and size() (Array<Vec4>: mip 0 as readTexture delivers it, six faces of size x size).
// `ProbeT` is EnvironmentProbe inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with `Vec3 sh_coefs[9]`
// (tests/cpp/lumix_compat_probes.h).
#pragma once

#include <math.h>
#include <string.h>

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "core/math.h"
	#include "renderer/render_module.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_probes.h"
#endif

namespace Lumix {

static_assert(sizeof(Vec4) == 16 && sizeof(Vec3) == 12, "a texel is four floats, a coefficient three");

struct GpuProbeBaker {
	enum { LEVELS = 5 }; // roughness_levels (:3704)
	struct Image { // one (face, level) of one reflection probe: size x size texels of r, g, b, m
		const u8* begin = nullptr;
		u32 bytes = 0, size = 0;
	};

	explicit GpuProbeBaker(LmxContext* ctx) : m_ctx(ctx) { lmx_probes_create(ctx, &m_baker); }
	~GpuProbeBaker() { lmx_probes_destroy(m_baker); }
	GpuProbeBaker(const GpuProbeBaker&) = delete;
	void operator=(const GpuProbeBaker&) = delete;

	// the callback of :3750-3757 for n jobs at once, then :3854-3858 for each
	template <typename JobT, typename ProbeT> bool bakeEnvironment(JobT* const* jobs, ProbeT* const* probes, u32 n) {
		if (!upload(jobs, n)) return false;
		if (lmx_probes_sh_run(m_baker) != LMX_OK) return false;
		m_coefs.resize(27 * (size_t)n);
		if (lmx_probes_read_sh(m_baker, m_coefs.data(), n) != LMX_OK) return false;
		for (u32 i = 0; i < n; ++i) {
			static_assert(sizeof(probes[i]->sh_coefs) == 27 * sizeof(float), "EnvironmentProbe::sh_coefs is Vec3[9]");
			memcpy(probes[i]->sh_coefs, m_coefs.data() + 27 * (size_t)i, sizeof(probes[i]->sh_coefs));
		}
		return true;
	}

	// :3685-3745 and saveCubemap's loop for n jobs at once
	template <typename JobT> bool bakeReflection(JobT* const* jobs, u32 n) {
		m_rgbm_jobs = 0;
		if (!upload(jobs, n)) return false;
		if (lmx_probes_filter_run(m_baker) != LMX_OK) return false;
		m_rgbm.resize(bytesPerProbe() * n);
		if (lmx_probes_read_rgbm(m_baker, m_rgbm.data(), m_rgbm.size()) != LMX_OK) return false;
		m_rgbm_jobs = n;
		return true;
	}

	// `memcpy(input.add(face, 0, level).pixels.getMutableData(), image.begin, image.bytes)` in saveCubemap's face / mip order
	Image rgbm(u32 job, u32 face, u32 level) const {
		Image img;
		if (job >= m_rgbm_jobs || face >= 6 || level >= LEVELS) return img;
		size_t at = bytesPerProbe() * job + bytesPerProbe() / 6 * face;
		for (u32 k = 0; k < level; ++k) at += 4 * (size_t)(m_size >> k) * (m_size >> k);
		img.size = m_size >> level;
		img.bytes = 4 * img.size * img.size;
		img.begin = m_rgbm.data() + at;
		return img;
	}

	bool getOutputs(LmxProbesDevice& out) const { return lmx_probes_device_outputs(m_baker, &out) == LMX_OK; }
	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxProbeBaker* handle() const { return m_baker; }

private:
	size_t bytesPerProbe() const {
		size_t texels = 0;
		for (u32 k = 0; k < LEVELS; ++k) texels += 6 * (size_t)(m_size >> k) * (m_size >> k);
		return 4 * texels;
	}

	// the captures of n jobs as one batch; every job holds 6 * size * size texels of one size (`w = (u32)sqrtf(len / 6.f)`, :550-552)
	template <typename JobT> bool upload(JobT* const* jobs, u32 n) {
		if (n == 0) return false;
		const size_t texels = (size_t)jobs[0]->data.size();
		const u32 size = (u32)sqrtf(texels / 6.f);
		if (size == 0 || 6 * (size_t)size * size != texels) return false;
		uint64_t bytes = 0;
		if (lmx_probes_batch_bytes(n, size, &bytes) != LMX_OK) return false;
		m_batch.resize((size_t)(bytes / sizeof(Vec4)));
		for (u32 i = 0; i < n; ++i) {
			if ((size_t)jobs[i]->data.size() != texels) return false;
			memcpy(m_batch.data() + texels * i, jobs[i]->data.begin(), texels * sizeof(Vec4));
		}
		m_size = size;
		return lmx_probes_set_cubemaps(m_baker, n, size, &m_batch[0].x) == LMX_OK;
	}

	LmxContext* m_ctx;
	LmxProbeBaker* m_baker = nullptr;
	u32 m_size = 0, m_rgbm_jobs = 0;
	std::vector<Vec4> m_batch;
	std::vector<float> m_coefs;
	std::vector<u8> m_rgbm;
};

} // namespace Lumix
