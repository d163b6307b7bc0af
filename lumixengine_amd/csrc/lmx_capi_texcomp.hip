// lmx_capi_texcomp.hip — the texture compressor's entry points (include/lumix_mi355.h, "Texture compressor"): what TextureCompressor::compress
// (renderer/editor/render_plugins.cpp:75-446) does per 4 x 4 block, as an object beside the context. The host side lays the batch out, builds
// the tables once and launches texcomp_kernels.hip; the arithmetic is lmx_texcomp.h's.
#include "lmx_context.h"
#include "lmx_texcomp.h"

#include <memory>
#include <new>

using namespace lmx;

struct LmxTexCompressor {
	LmxContext* ctx = nullptr;
	uint32_t n_images = 0, n_blocks = 0; // the batch of the last set
	int format = -1;                     // of the last run on this batch; -1: none
	bool images_in_flight = false;       // h_images was handed to an on-stream copy no synchronize has followed yet
	std::vector<TcImage> h_images;
	const uint32_t* d_rgba = nullptr; // d_own.p, or the caller's / the probe baker's pixels
	DevBuf<TcImage> d_images;
	DevBuf<uint32_t> d_own, d_out;
	DevBuf<TcTables> d_tables;
};

namespace {

constexpr size_t TC_GUARD_WORDS = 64; // behind the blocks of a run: filled, never written by a kernel (lmx_context.h, fill_guard)

#define LMX_TEXCOMP_ENTER(tc)                          \
	if (!(tc)) return LMX_ERR_INVALID_ARGUMENT;        \
	LmxContext* ctx = (tc)->ctx;                       \
	LMX_CHECK_CTX(ctx)

uint32_t words_per_block(int format) { return format == LMX_TEX_BC1 || format == LMX_TEX_BC4 ? 2u : 4u; }
bool format_ok(int format) { return format == LMX_TEX_BC1 || format == LMX_TEX_BC3 || format == LMX_TEX_BC4 || format == LMX_TEX_BC5; }

// the batch's layout from its descriptors; `what`: what was wrong, for the message
int lay_out(uint32_t n, const LmxTexImage* descs, std::vector<TcImage>* images, uint64_t* pixels, uint64_t* blocks, const char** what) {
	*pixels = *blocks = 0;
	*what = "";
	if (n == 0 || !descs) {
		*what = "an empty batch or null descriptors";
		return LMX_ERR_INVALID_ARGUMENT;
	}
	for (uint32_t i = 0; i < n; ++i)
		if (descs[i].w == 0 || descs[i].h == 0) {
			*what = "an image with a zero dimension";
			return LMX_ERR_INVALID_ARGUMENT;
		}
	if (images) {
		try {
			images->resize(n);
		} catch (const std::bad_alloc&) {
			*what = "host allocation of the batch's descriptors failed";
			return LMX_ERR_OUT_OF_MEMORY;
		}
	}
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t px = (uint64_t)descs[i].w * descs[i].h;
		if (px > LMX_TEXCOMP_MAX_BATCH_BYTES / 4 || (*pixels + px) * 4 > LMX_TEXCOMP_MAX_BATCH_BYTES) {
			*what = "a batch above LMX_TEXCOMP_MAX_BATCH_BYTES";
			return LMX_ERR_CAPACITY;
		}
		if (images) (*images)[i] = TcImage{descs[i].w, descs[i].h, (uint32_t)*pixels, (uint32_t)*blocks};
		*pixels += px;
		*blocks += (uint64_t)((descs[i].w + 3) >> 2) * ((descs[i].h + 3) >> 2); // (<= 2^28 pixels: at most 2^28 blocks)
	}
	return LMX_OK;
}

// the descriptors of a new batch go up on the stream, without a host wait unless the batch before is still being copied
int take_batch(LmxTexCompressor* tc, uint32_t n, const LmxTexImage* descs, uint64_t* pixels) {
	LmxContext* ctx = tc->ctx;
	std::vector<TcImage> images;
	uint64_t blocks;
	const char* what;
	if (int rc = lay_out(n, descs, &images, pixels, &blocks, &what)) return fail(ctx, rc, "texcomp: %s", what);
	if (tc->images_in_flight || tc->d_images.cap < n) { // (the copy still reads h_images; a queued kernel may still read the table a reserve frees)
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		tc->images_in_flight = false;
	}
	tc->n_images = tc->n_blocks = 0;
	tc->format = -1;
	tc->h_images.swap(images);
	LMX_HIP(ctx, upload_on_stream(tc->d_images, tc->h_images.data(), (size_t)n, ctx->stream));
	tc->images_in_flight = true;
	tc->n_images = n;
	tc->n_blocks = (uint32_t)blocks;
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_texcomp_output_bytes(uint32_t n, const LmxTexImage* descs, int format, uint64_t* out) {
	if (!out) return LMX_ERR_INVALID_ARGUMENT;
	*out = 0;
	if (!format_ok(format)) return LMX_ERR_INVALID_ARGUMENT;
	uint64_t pixels, blocks;
	const char* what;
	if (int rc = lay_out(n, descs, nullptr, &pixels, &blocks, &what)) return rc;
	*out = blocks * words_per_block(format) * 4;
	return LMX_OK;
}

uint32_t lmx_texcomp_blocks_per_round(void) { return TC_BLOCKS_PER_ROUND; }

int lmx_texcomp_tables(void* out, uint64_t cap_bytes) {
	if (!out || cap_bytes < sizeof(TcTables)) return LMX_ERR_INVALID_ARGUMENT;
	std::unique_ptr<TcTables> t(new (std::nothrow) TcTables());
	if (!t) return LMX_ERR_OUT_OF_MEMORY;
	tc_build_tables(t.get());
	memcpy(out, t.get(), sizeof(TcTables));
	return LMX_OK;
}

int lmx_texcomp_hist_index(uint32_t colours, const uint8_t* hist, uint32_t* out) {
	if (!hist || !out || (colours != 3 && colours != 4)) return LMX_ERR_INVALID_ARGUMENT;
	uint32_t sum = 0;
	for (uint32_t i = 0; i < colours; ++i) sum += hist[i];
	if (sum != 16) return LMX_ERR_INVALID_ARGUMENT;
	*out = tc_hist_index(colours, hist);
	return LMX_OK;
}

int lmx_texcomp_encode_host(int format, uint32_t n_blocks, const uint8_t* rgba, uint8_t* out, uint32_t* err) {
	if (!format_ok(format) || !rgba || !out) return LMX_ERR_INVALID_ARGUMENT;
	std::unique_ptr<TcTables> t(new (std::nothrow) TcTables());
	if (!t) return LMX_ERR_OUT_OF_MEMORY;
	tc_build_tables(t.get());
	const uint32_t words = words_per_block(format);
	for (uint32_t b = 0; b < n_blocks; ++b) {
		uint32_t px[16], w[4] = {0, 0, 0, 0}, e = 0;
		memcpy(px, rgba + 64 * (size_t)b, 64);
		if (format == LMX_TEX_BC1) {
			const TcBlock c = tc_encode_bc1_host(px, true, *t, &e);
			w[0] = c.w0, w[1] = c.w1;
		} else if (format == LMX_TEX_BC3) {
			const TcBlock a = tc_encode_bc4(px, 24), c = tc_encode_bc1_host(px, false, *t, &e);
			w[0] = a.w0, w[1] = a.w1, w[2] = c.w0, w[3] = c.w1;
		} else {
			const TcBlock a = tc_encode_bc4(px, 0), c = tc_encode_bc4(px, 8);
			w[0] = a.w0, w[1] = a.w1, w[2] = c.w0, w[3] = c.w1;
		}
		memcpy(out + 4 * (size_t)words * b, w, 4 * (size_t)words);
		if (err) err[b] = e;
	}
	return LMX_OK;
}

int lmx_texcomp_create(LmxContext* ctx, LmxTexCompressor** out) {
	LMX_CHECK_CTX(ctx);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	*out = nullptr;
	std::unique_ptr<LmxTexCompressor> tc(new (std::nothrow) LmxTexCompressor());
	std::unique_ptr<TcTables> t(new (std::nothrow) TcTables());
	if (!tc || !t) return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "texcomp: host allocation failed");
	tc->ctx = ctx;
	tc_build_tables(t.get());
	if (int rc = upload_settled(ctx, tc->d_tables, (const TcTables*)t.get(), (size_t)1)) return rc;
	*out = tc.release();
	return LMX_OK;
}

void lmx_texcomp_destroy(LmxTexCompressor* tc) {
	if (!tc) return;
	(void)hipSetDevice(tc->ctx->device);
	(void)hipStreamSynchronize(tc->ctx->stream);
	delete tc;
}

int lmx_texcomp_set_images(LmxTexCompressor* tc, uint32_t n, const LmxTexImage* descs, const uint8_t* rgba) {
	LMX_TEXCOMP_ENTER(tc);
	if (n && descs && !rgba) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null pixels");
	uint64_t pixels;
	if (int rc = take_batch(tc, n, descs, &pixels)) return rc;
	tc->d_rgba = nullptr;
	const uint32_t n_blocks = tc->n_blocks;
	tc->n_images = tc->n_blocks = 0; // (until the pixels are up)
	// upload_settled's pair of synchronizes around a copy of bytes: the caller's array need not be aligned to words, the device's is
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, tc->d_own.reserve((size_t)pixels));
	LMX_HIP(ctx, upload_on_stream(reinterpret_cast<uint8_t*>(tc->d_own.p), rgba, 4 * (size_t)pixels, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	tc->images_in_flight = false; // (the stream has drained)
	tc->d_rgba = tc->d_own.p;
	tc->n_images = n;
	tc->n_blocks = n_blocks;
	return LMX_OK;
}

int lmx_texcomp_set_images_device(LmxTexCompressor* tc, uint32_t n, const LmxTexImage* descs, const uint8_t* d_rgba) {
	LMX_TEXCOMP_ENTER(tc);
	if (n && descs && !d_rgba) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null device pixels");
	if ((uintptr_t)d_rgba & 3u) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: device pixels are read as 32-bit words: the pointer must be a multiple of 4");
	uint64_t pixels;
	if (int rc = take_batch(tc, n, descs, &pixels)) return rc;
	tc->d_rgba = reinterpret_cast<const uint32_t*>(d_rgba);
	return LMX_OK;
}

int lmx_texcomp_set_from_probes(LmxTexCompressor* tc, LmxProbeBaker* pb) {
	LMX_TEXCOMP_ENTER(tc);
	if (!pb) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null probe baker");
	LmxProbesDevice dev;
	if (int rc = lmx_probes_device_outputs(pb, &dev)) return rc == LMX_ERR_NOT_BUILT ? fail(ctx, rc, "texcomp: set_from_probes before filter_run") : rc;
	if (!dev.d_rgbm) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: set_from_probes before filter_run");
	constexpr uint32_t LEVELS = 5; // saveCubemap's roughness levels: per probe, per face, levels 0 .. 4 (:3555-3559)
	std::vector<LmxTexImage> descs;
	try {
		descs.reserve((size_t)dev.n * 6 * LEVELS);
	} catch (const std::bad_alloc&) {
		return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "texcomp: host allocation of the batch's descriptors failed");
	}
	for (uint32_t p = 0; p < dev.n; ++p)
		for (uint32_t face = 0; face < 6; ++face)
			for (uint32_t level = 0; level < LEVELS; ++level) descs.push_back(LmxTexImage{dev.size >> level, dev.size >> level});
	uint64_t pixels;
	if (int rc = take_batch(tc, (uint32_t)descs.size(), descs.data(), &pixels)) return rc;
	tc->d_rgba = reinterpret_cast<const uint32_t*>(dev.d_rgbm);
	return LMX_OK;
}

int lmx_texcomp_run(LmxTexCompressor* tc, int format) {
	LMX_TEXCOMP_ENTER(tc);
	if (!format_ok(format)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: unknown format %d", format);
	if (!tc->n_images || !tc->d_rgba) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: run before a batch was set");
	const uint32_t stride = words_per_block(format);
	const size_t words = (size_t)tc->n_blocks * stride;
	if (tc->d_out.cap < words + TC_GUARD_WORDS) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a queued kernel may still write the buffer a reserve frees)
		LMX_HIP(ctx, tc->d_out.reserve(words + TC_GUARD_WORDS));
	}
	tc->format = -1;
	LMX_HIP(ctx, fill_guard(tc->d_out.p + words, TC_GUARD_WORDS, ctx->stream));
	const TcBatch batch{tc->d_images.p, tc->d_rgba, tc->n_images, tc->n_blocks};
	switch (format) {
		case LMX_TEX_BC1: LMX_HIP(ctx, launch_bc1_search(ctx->stream, batch, tc->d_tables.p, true, tc->d_out.p, stride, 0)); break;
		case LMX_TEX_BC3:
			LMX_HIP(ctx, launch_bc4(ctx->stream, batch, 1, 24, 24, tc->d_out.p, stride));
			LMX_HIP(ctx, launch_bc1_search(ctx->stream, batch, tc->d_tables.p, false, tc->d_out.p, stride, 2));
			break;
		case LMX_TEX_BC4: LMX_HIP(ctx, launch_bc4(ctx->stream, batch, 1, 0, 0, tc->d_out.p, stride)); break;
		case LMX_TEX_BC5: LMX_HIP(ctx, launch_bc4(ctx->stream, batch, 2, 0, 8, tc->d_out.p, stride)); break; // encode_bc5's defaults: channels 0 and 1
	}
	tc->format = format;
	return LMX_OK;
}

int lmx_texcomp_read(LmxTexCompressor* tc, uint8_t* out, uint64_t cap_bytes) {
	LMX_TEXCOMP_ENTER(tc);
	if (tc->format < 0) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: no run on this batch");
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	const size_t used = (size_t)tc->n_blocks * words_per_block(tc->format) * 4;
	const int rc = read_out(ctx, out, (size_t)cap_bytes, reinterpret_cast<const uint8_t*>(tc->d_out.p), used, used + 4 * TC_GUARD_WORDS, "bytes of blocks");
	if (rc == LMX_OK) tc->images_in_flight = false; // (the read drained the stream)
	return rc;
}

int lmx_texcomp_device_outputs(LmxTexCompressor* tc, LmxTexCompDevice* out) {
	LMX_TEXCOMP_ENTER(tc);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!tc->n_images) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: no batch");
	out->d_rgba = reinterpret_cast<const uint8_t*>(tc->d_rgba);
	out->d_blocks = tc->format < 0 ? nullptr : reinterpret_cast<const uint8_t*>(tc->d_out.p);
	out->bytes = tc->format < 0 ? 0 : (uint64_t)tc->n_blocks * words_per_block(tc->format) * 4;
	out->n_images = tc->n_images;
	out->n_blocks = tc->n_blocks;
	out->format = tc->format;
	return LMX_OK;
}

} // extern "C"
