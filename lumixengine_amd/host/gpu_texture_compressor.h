// gpu_texture_compressor.h — the texture compressor's host adapter (C++ host side of include/lumix_mi355.h "Texture compressor").
//
// In the reference TextureCompressor::compress (src/renderer/editor/render_plugins.cpp:415-444) picks the format, writes the LBCHeader and
// runs one of compressBC1 / compressBC3 / compressBC5 over every image in slice, face, mip order (:372-374), each a jobs::forEach over block
// rows calling rgbcx per block. GpuTextureCompressor::compress does the same with the block loops on the device:
//   - the format choice (:423-427): a size not divisible by 4, or options.compress off, stays RGBA8 - the images are appended as they are, a
//     host copy (the reference appends them and then, its `if` chain having no `else`, the blocks of an encoder reading stale rows as well:
//     not followed); is_normalmap -> BC5, has_alpha -> BC3, else BC1;
//   - the LBCHeader (writeLBCHeader, :312-322);
//   - the images in the loop's order as one batch, one lmx_texcomp_run, the blocks appended behind the header.
// With options.generate_mipmaps set compress returns false, as it does wherever the library refuses (lastError() says why): such an input
// goes to compressWithMips, which has the chains built on the device (computeMip, computeCoverage, scaleCoverage: DESIGN.md §4.24) and
// compresses them where they lie.
//
// `InputT` is TextureCompressor::Input-shaped (w, h, slices, mips, is_normalmap, has_alpha, is_cubemap, has(face, slice, mip) and
// get(face, slice, mip).pixels with data() and size()), `OptionsT` Options-shaped (compress, generate_mipmaps), `StreamT`
// OutputMemoryStream-shaped (write(ptr, bytes), size(), resize(bytes), getMutableData()): the reference keeps the first two private to
// render_plugins.cpp. LBCHeader and gpu::TextureFormat are the engine's inside it (-DLMX_WITH_LUMIX_HEADERS); a standalone build takes them
// from tests/cpp/lumix_compat_texcomp.h.
#pragma once

#include <string.h>

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "renderer/gpu/gpu.h"
	#include "renderer/texture.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_texcomp.h"
#endif

namespace Lumix {

struct GpuTextureCompressor {
	explicit GpuTextureCompressor(LmxContext* ctx) : m_ctx(ctx) { lmx_texcomp_create(ctx, &m_tc); }
	~GpuTextureCompressor() { lmx_texcomp_destroy(m_tc); }
	GpuTextureCompressor(const GpuTextureCompressor&) = delete;
	void operator=(const GpuTextureCompressor&) = delete;

	// the format compress() writes for this input (:423-427)
	template <typename InputT, typename OptionsT> static gpu::TextureFormat formatOf(const InputT& src, const OptionsT& options) {
		const bool can_compress = options.compress && (src.w % 4) == 0 && (src.h % 4) == 0;
		if (!can_compress) return gpu::TextureFormat::RGBA8;
		if (src.is_normalmap) return gpu::TextureFormat::BC5;
		if (src.has_alpha) return gpu::TextureFormat::BC3;
		return gpu::TextureFormat::BC1;
	}

	// TextureCompressor::compress(src, options, dst, allocator) for options.generate_mipmaps == false
	template <typename InputT, typename OptionsT, typename StreamT> bool compress(const InputT& src, const OptionsT& options, StreamT& dst) {
		if (!m_tc || options.generate_mipmaps) return false;
		const u32 faces = src.is_cubemap ? 6u : 1u;
		for (u32 mip = 0; mip < src.mips; ++mip) // isValid (:403-413)
			for (u32 slice = 0; slice < src.slices; ++slice)
				for (u32 face = 0; face < faces; ++face)
					if (!src.has(face, slice, mip)) return false;
		const gpu::TextureFormat format = formatOf(src, options);
		m_descs.clear();
		size_t bytes = 0;
		for (u32 slice = 0; slice < src.slices; ++slice)
			for (u32 face = 0; face < faces; ++face)
				for (u32 mip = 0; mip < src.mips; ++mip) {
					const LmxTexImage d = {mipSize(src.w, mip), mipSize(src.h, mip)};
					if ((size_t)src.get(face, slice, mip).pixels.size() != 4 * (size_t)d.w * d.h) return false;
					m_descs.push_back(d);
					bytes += 4 * (size_t)d.w * d.h;
				}
		if (m_descs.empty()) return false;
		int lmx_format = LMX_TEX_BC1;
		if (format == gpu::TextureFormat::BC5) lmx_format = LMX_TEX_BC5;
		else if (format == gpu::TextureFormat::BC3) lmx_format = LMX_TEX_BC3;
		uint64_t out_bytes = 0;
		if (format != gpu::TextureFormat::RGBA8) {
			// (everything that can refuse comes before the first byte is written: a false return leaves dst as it was)
			if (lmx_texcomp_output_bytes((u32)m_descs.size(), m_descs.data(), lmx_format, &out_bytes) != LMX_OK) return false;
			m_batch.resize(bytes);
			size_t at = 0;
			for (u32 slice = 0; slice < src.slices; ++slice)
				for (u32 face = 0; face < faces; ++face)
					for (u32 mip = 0; mip < src.mips; ++mip) {
						const auto& pixels = src.get(face, slice, mip).pixels;
						memcpy(m_batch.data() + at, pixels.data(), (size_t)pixels.size());
						at += (size_t)pixels.size();
					}
			if (lmx_texcomp_set_images(m_tc, (u32)m_descs.size(), m_descs.data(), m_batch.data()) != LMX_OK) return false;
			if (lmx_texcomp_run(m_tc, lmx_format) != LMX_OK) return false;
		}
		LBCHeader header; // writeLBCHeader (:312-322)
		header.w = src.w;
		header.h = src.h;
		header.slices = src.slices;
		header.mips = src.mips;
		header.format = format;
		if (src.is_cubemap) header.flags |= LBCHeader::CUBEMAP;
		const size_t start = (size_t)dst.size();
		dst.write(&header, sizeof(header));
		if (format == gpu::TextureFormat::RGBA8) {
			for (u32 slice = 0; slice < src.slices; ++slice)
				for (u32 face = 0; face < faces; ++face)
					for (u32 mip = 0; mip < src.mips; ++mip) {
						const auto& pixels = src.get(face, slice, mip).pixels;
						dst.write(pixels.data(), pixels.size());
					}
			return true;
		}
		const size_t payload = (size_t)dst.size();
		dst.resize(payload + (size_t)out_bytes);
		if (lmx_texcomp_read(m_tc, (uint8_t*)dst.getMutableData() + payload, out_bytes) != LMX_OK) {
			dst.resize(start);
			return false;
		}
		return true;
	}

	// TextureCompressor::compress(src, options, dst, allocator) for options.generate_mipmaps == true (:359-401): the chains are built on the
	// device - computeMip by options.stochastic_mipmap / src.is_srgb, scaleCoverage for options.scale_coverage_ref >= 0 - and compressed
	// where they lie. `OptionsT` has stochastic_mipmap and scale_coverage_ref besides, `InputT` is_srgb. A size that stays RGBA8 gets the
	// chains' pixels as its payload. A false return leaves dst as it was.
	template <typename InputT, typename OptionsT, typename StreamT> bool compressWithMips(const InputT& src, const OptionsT& options, StreamT& dst) {
		if (!m_tc || !options.generate_mipmaps || src.mips != 1) return false; // isValid (:403-413): generated chains start from one mip
		const u32 faces = src.is_cubemap ? 6u : 1u;
		for (u32 slice = 0; slice < src.slices; ++slice)
			for (u32 face = 0; face < faces; ++face)
				if (!src.has(face, slice, 0)) return false;
		const gpu::TextureFormat format = formatOf(src, options);
		const u32 mips = lmx_texcomp_chain_levels(src.w, src.h); // 1 + log2(maximum(w, h)) (:420)
		const u32 n = src.slices * faces;
		uint64_t chain_bytes = 0, out_bytes = 0;
		// (everything that can refuse comes before the first byte is written)
		if (!mips || !n || lmx_texcomp_chain_bytes(n, src.w, src.h, &chain_bytes) != LMX_OK) return false;
		const size_t image_bytes = 4 * (size_t)src.w * src.h;
		m_batch.resize(image_bytes * n);
		size_t at = 0;
		for (u32 slice = 0; slice < src.slices; ++slice)
			for (u32 face = 0; face < faces; ++face) {
				const auto& pixels = src.get(face, slice, 0).pixels;
				if ((size_t)pixels.size() != image_bytes) return false;
				memcpy(m_batch.data() + at, pixels.data(), image_bytes);
				at += image_bytes;
			}
		LmxTexMipOptions mip_options;
		mip_options.mode = options.stochastic_mipmap ? LMX_TEXMIP_STOCHASTIC : src.is_srgb ? LMX_TEXMIP_SRGB : LMX_TEXMIP_LINEAR; // computeMip's order (:202-215)
		mip_options.scale_coverage_ref = options.scale_coverage_ref;
		int lmx_format = LMX_TEX_BC1;
		if (format == gpu::TextureFormat::BC5) lmx_format = LMX_TEX_BC5;
		else if (format == gpu::TextureFormat::BC3) lmx_format = LMX_TEX_BC3;
		if (format != gpu::TextureFormat::RGBA8) {
			m_descs.clear();
			for (u32 i = 0; i < n; ++i)
				for (u32 mip = 0; mip < mips; ++mip) m_descs.push_back(LmxTexImage{mipSize(src.w, mip), mipSize(src.h, mip)});
			if (lmx_texcomp_output_bytes((u32)m_descs.size(), m_descs.data(), lmx_format, &out_bytes) != LMX_OK) return false;
		}
		if (lmx_texcomp_set_chains(m_tc, n, src.w, src.h, m_batch.data()) != LMX_OK) return false;
		if (lmx_texcomp_generate_mips(m_tc, &mip_options) != LMX_OK) return false;
		if (format != gpu::TextureFormat::RGBA8 && lmx_texcomp_run(m_tc, lmx_format) != LMX_OK) return false;
		LBCHeader header; // writeLBCHeader (:312-322)
		header.w = src.w;
		header.h = src.h;
		header.slices = src.slices;
		header.mips = mips;
		header.format = format;
		if (src.is_cubemap) header.flags |= LBCHeader::CUBEMAP;
		const size_t start = (size_t)dst.size();
		dst.write(&header, sizeof(header));
		const size_t payload = (size_t)dst.size();
		const uint64_t bytes = format == gpu::TextureFormat::RGBA8 ? chain_bytes : out_bytes;
		dst.resize(payload + (size_t)bytes);
		uint8_t* out = (uint8_t*)dst.getMutableData() + payload;
		const int rc = format == gpu::TextureFormat::RGBA8 ? lmx_texcomp_read_pixels(m_tc, out, bytes) : lmx_texcomp_read(m_tc, out, bytes);
		if (rc != LMX_OK) {
			dst.resize(start);
			return false;
		}
		return true;
	}

	static u32 mipSize(u32 v, u32 mip) { return (v >> mip) > 1u ? (v >> mip) : 1u; } // maximum(v >> mip, 1) (:375-376)
	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxTexCompressor* handle() const { return m_tc; }

private:
	LmxContext* m_ctx;
	LmxTexCompressor* m_tc = nullptr;
	std::vector<LmxTexImage> m_descs;
	std::vector<u8> m_batch;
};

} // namespace Lumix
