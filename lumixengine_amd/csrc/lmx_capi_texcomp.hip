// lmx_capi_texcomp.hip — the texture compressor's entry points (include/lumix_mi355.h, "Texture compressor"): what TextureCompressor::compress
// (renderer/editor/render_plugins.cpp:75-446) does per 4 x 4 block, as an object beside the context. The host side lays the batch out, builds
// the tables once and launches texcomp_kernels.hip; the arithmetic is lmx_texcomp.h's.
#include "lmx_context.h"
#include "lmx_texcomp.h"
#include "lmx_texmips.h"

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
	// mip chains (lmx_texmips.h): the batch is chain_n chains of chain_w x chain_h level-0 images, in d_own
	bool chains = false, mips_done = false;
	uint32_t chain_n = 0, chain_w = 0, chain_h = 0;
	std::vector<TmRow> h_rows;       // per generated level: the taps of its columns, then of its rows (uploaded with h_images)
	std::vector<uint32_t> rows_at;   // of level m in h_rows / d_rows; [0] unused
	std::vector<uint32_t> windows;   // per level: the largest source window of a tile along x, along y
	DevBuf<TmRow> d_rows;
	DevBuf<TmTables> d_mip_tables;
	DevBuf<uint32_t> d_hist;         // coverage: 256 bins per chain for each level made by a launch of its own, then computeCoverage's count
};

namespace {

constexpr size_t TC_GUARD_WORDS = 64; // behind the blocks of a run: filled, never written by a kernel (lmx_context.h, fill_guard)

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

// the search tables and the mip filter's, built on the host once per compressor
int upload_tables(LmxTexCompressor* tc) {
	LmxContext* ctx = tc->ctx;
	std::unique_ptr<TcTables> t(new (std::nothrow) TcTables());
	if (!t) return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "texcomp: host allocation failed");
	tc_build_tables(t.get());
	if (int rc = upload_settled(ctx, tc->d_tables, (const TcTables*)t.get(), (size_t)1)) return rc;
	TmTables mip_tables;
	tm_build_tables(&mip_tables);
	return upload_settled(ctx, tc->d_mip_tables, (const TmTables*)&mip_tables, (size_t)1);
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
	tc->chains = tc->mips_done = false;
	tc->h_images.swap(images);
	LMX_HIP(ctx, upload_on_stream(tc->d_images, tc->h_images.data(), (size_t)n, ctx->stream));
	tc->images_in_flight = true;
	tc->n_images = n;
	tc->n_blocks = (uint32_t)blocks;
	return LMX_OK;
}

// ---- mip chains -----------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t TM_MAX_CHAINS = 65535; // the chain is a grid dimension of the level kernels

bool mode_ok(int mode) { return mode == LMX_TEXMIP_LINEAR || mode == LMX_TEXMIP_SRGB || mode == LMX_TEXMIP_STOCHASTIC; }

// n chains of w x h: their pixels, or what is wrong with them
int chains_lay_out(uint32_t n, uint32_t w, uint32_t h, uint64_t* pixels, const char** what) {
	*pixels = 0;
	*what = "";
	if (n == 0 || w == 0 || h == 0) {
		*what = "no chain, or a zero side";
		return LMX_ERR_INVALID_ARGUMENT;
	}
	constexpr uint64_t cap_px = LMX_TEXCOMP_MAX_BATCH_BYTES / 4;
	if (w > TM_MAX_SIDE || h > TM_MAX_SIDE) {
		*what = "a side above 2^24 (a texel centre is no longer exact in fp32)";
		return LMX_ERR_CAPACITY;
	}
	if ((uint64_t)w * h > cap_px || tm_chain_pixels(w, h) > cap_px || tm_chain_pixels(w, h) * n > cap_px) {
		*what = "chains above LMX_TEXCOMP_MAX_BATCH_BYTES";
		return LMX_ERR_CAPACITY;
	}
	if (n > TM_MAX_CHAINS) {
		*what = "more than 65535 chains";
		return LMX_ERR_CAPACITY;
	}
	*pixels = tm_chain_pixels(w, h) * n;
	return LMX_OK;
}

// the taps of every generated level of a w x h chain, and the windows their tiles need
bool chain_rows(uint32_t w, uint32_t h, std::vector<TmRow>* rows, std::vector<uint32_t>* rows_at, std::vector<uint32_t>* windows) {
	const uint32_t levels = tm_levels(w, h);
	size_t total = 0;
	rows_at->assign(levels, 0);
	windows->assign(2 * (size_t)levels, 0);
	for (uint32_t m = 1; m < levels; ++m) {
		(*rows_at)[m] = (uint32_t)total;
		total += (size_t)tm_side(w, m) + tm_side(h, m);
	}
	rows->resize(total);
	for (uint32_t m = 1; m < levels; ++m) {
		TmRow* rx = rows->data() + (*rows_at)[m];
		TmRow* ry = rx + tm_side(w, m);
		if (!tm_build_coeffs(tm_side(w, m - 1), tm_side(w, m), rx) || !tm_build_coeffs(tm_side(h, m - 1), tm_side(h, m), ry)) return false;
		(*windows)[2 * m] = tm_max_window(rx, tm_side(w, m));
		(*windows)[2 * m + 1] = tm_max_window(ry, tm_side(h, m));
		if ((*windows)[2 * m] > TM_WINDOW || (*windows)[2 * m + 1] > TM_WINDOW) return false;
	}
	return true;
}

int set_chains(LmxTexCompressor* tc, uint32_t n, uint32_t w, uint32_t h, const uint8_t* rgba, bool on_device) {
	LmxContext* ctx = tc->ctx;
	if (!rgba) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null pixels");
	if (on_device && ((uintptr_t)rgba & 3u)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: device pixels are read as 32-bit words: the pointer must be a multiple of 4");
	uint64_t chain_pixels;
	const char* what;
	if (int rc = chains_lay_out(n, w, h, &chain_pixels, &what)) return fail(ctx, rc, "texcomp: %s", what);
	const uint32_t levels = tm_levels(w, h);
	const size_t chain_px = (size_t)tm_chain_pixels(w, h);
	std::vector<LmxTexImage> descs;
	std::vector<TmRow> rows;
	std::vector<uint32_t> rows_at, windows;
	try {
		descs.reserve((size_t)n * levels);
		for (uint32_t i = 0; i < n; ++i)
			for (uint32_t m = 0; m < levels; ++m) descs.push_back(LmxTexImage{tm_side(w, m), tm_side(h, m)});
		if (!chain_rows(w, h, &rows, &rows_at, &windows)) return fail(ctx, LMX_ERR_UNSUPPORTED, "texcomp: a level of a %u x %u chain needs more taps or a wider window than the kernels hold", w, h);
	} catch (const std::bad_alloc&) {
		return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "texcomp: host allocation of the chains' tables failed");
	}
	// the stream drains only where a reserve below would free a buffer queued kernels may still use (take_batch does the same for the
	// descriptors, and waits where the tables of the set before are still being copied: h_rows goes up with h_images)
	if (tc->d_rows.cap < std::max<size_t>(rows.size(), 1) || tc->d_own.cap < (size_t)chain_pixels + TC_GUARD_WORDS) {
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		tc->images_in_flight = false;
	}
	uint64_t pixels;
	if (int rc = take_batch(tc, (uint32_t)descs.size(), descs.data(), &pixels)) return rc;
	const uint32_t n_images = tc->n_images, n_blocks = tc->n_blocks;
	tc->n_images = tc->n_blocks = 0; // (until the pixels are up)
	tc->d_rgba = nullptr;
	tc->h_rows.swap(rows);
	tc->rows_at.swap(rows_at);
	tc->windows.swap(windows);
	LMX_HIP(ctx, upload_on_stream(tc->d_rows, tc->h_rows, ctx->stream));
	LMX_HIP(ctx, tc->d_own.reserve((size_t)pixels + TC_GUARD_WORDS));
	LMX_HIP(ctx, fill_guard(tc->d_own.p + pixels, TC_GUARD_WORDS, ctx->stream));
	// every level 0 to the head of its chain: one strided copy
	const size_t image_bytes = 4 * (size_t)w * h;
	LMX_HIP(ctx, hipMemcpy2DAsync(tc->d_own.p, 4 * chain_px, rgba, image_bytes, image_bytes, n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
	if (!on_device) { // (the caller's array has been read when this returns)
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		tc->images_in_flight = false;
	}
	tc->d_rgba = tc->d_own.p;
	tc->n_images = n_images;
	tc->n_blocks = n_blocks;
	tc->chains = true;
	tc->chain_n = n;
	tc->chain_w = w;
	tc->chain_h = h;
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
	if (int rc = object_create(ctx, out, "texcomp")) return rc;
	const int rc = upload_tables(*out);
	if (rc) { // (no handle to an object without its tables)
		object_destroy(*out);
		*out = nullptr;
	}
	return rc;
}

void lmx_texcomp_destroy(LmxTexCompressor* tc) {
	if (tc) object_destroy(tc);
}

int lmx_texcomp_set_images(LmxTexCompressor* tc, uint32_t n, const LmxTexImage* descs, const uint8_t* rgba) {
	LMX_ENTER(tc);
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
	LMX_ENTER(tc);
	if (n && descs && !d_rgba) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null device pixels");
	if ((uintptr_t)d_rgba & 3u) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: device pixels are read as 32-bit words: the pointer must be a multiple of 4");
	uint64_t pixels;
	if (int rc = take_batch(tc, n, descs, &pixels)) return rc;
	tc->d_rgba = reinterpret_cast<const uint32_t*>(d_rgba);
	return LMX_OK;
}

int lmx_texcomp_set_from_probes(LmxTexCompressor* tc, LmxProbeBaker* pb) {
	LMX_ENTER(tc);
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
	LMX_ENTER(tc);
	if (!format_ok(format)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: unknown format %d", format);
	if (!tc->n_images || !tc->d_rgba) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: run before a batch was set");
	if (tc->chains && !tc->mips_done) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: run on chains before generate_mips");
	const uint32_t stride = words_per_block(format);
	const size_t words = (size_t)tc->n_blocks * stride;
	if (int rc = Grow{ctx}(tc->d_out, words + TC_GUARD_WORDS)) return rc;
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
	LMX_ENTER(tc);
	if (tc->format < 0) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: no run on this batch");
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	const size_t used = (size_t)tc->n_blocks * words_per_block(tc->format) * 4;
	const int rc = read_out(ctx, out, (size_t)cap_bytes, reinterpret_cast<const uint8_t*>(tc->d_out.p), used, used + 4 * TC_GUARD_WORDS, "bytes of blocks");
	if (rc == LMX_OK) tc->images_in_flight = false; // (the read drained the stream)
	return rc;
}

int lmx_texcomp_device_outputs(LmxTexCompressor* tc, LmxTexCompDevice* out) {
	LMX_ENTER(tc);
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

// ---- mip chains -----------------------------------------------------------------------------------------------------------------------------
uint32_t lmx_texcomp_chain_levels(uint32_t w, uint32_t h) { return w && h ? tm_levels(w, h) : 0u; }

int lmx_texcomp_chain_bytes(uint32_t n, uint32_t w, uint32_t h, uint64_t* out) {
	if (!out) return LMX_ERR_INVALID_ARGUMENT;
	*out = 0;
	uint64_t pixels;
	const char* what;
	if (int rc = chains_lay_out(n, w, h, &pixels, &what)) return rc;
	*out = pixels * 4;
	return LMX_OK;
}

int lmx_texcomp_set_chains(LmxTexCompressor* tc, uint32_t n, uint32_t w, uint32_t h, const uint8_t* rgba) {
	LMX_ENTER(tc);
	return set_chains(tc, n, w, h, rgba, false);
}

int lmx_texcomp_set_chains_device(LmxTexCompressor* tc, uint32_t n, uint32_t w, uint32_t h, const uint8_t* d_rgba) {
	LMX_ENTER(tc);
	return set_chains(tc, n, w, h, d_rgba, true);
}

int lmx_texcomp_generate_mips(LmxTexCompressor* tc, const LmxTexMipOptions* options) {
	LMX_ENTER(tc);
	if (!options) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: null options");
	if (!mode_ok(options->mode)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "texcomp: unknown mip mode %d", options->mode);
	if (!tc->chains) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: generate_mips without set_chains");
	const uint32_t w = tc->chain_w, h = tc->chain_h, n = tc->chain_n, levels = tm_levels(w, h);
	if (options->mode == LMX_TEXMIP_STOCHASTIC && (w > TM_STOCHASTIC_MAX_SIDE || h > TM_STOCHASTIC_MAX_SIDE))
		return fail(ctx, LMX_ERR_CAPACITY, "texcomp: a stochastic chain of %u x %u: above %u the reference's own index can leave a row", w, h, TM_STOCHASTIC_MAX_SIDE);
	const bool coverage = options->scale_coverage_ref >= 0.0f && levels > 1;
	const uint32_t chain_px = (uint32_t)tm_chain_pixels(w, h);
	tc->format = -1; // (the blocks of a run before are of other pixels)
	tc->mips_done = false;
	// levels 1 .. first_small by one launch each; the levels behind first_small, whose sides are both at most TM_TAIL_SIDE, by one k_mip_tail
	const uint32_t first_small = tm_tail_level(w, h, TM_TAIL_SIDE);
	uint32_t* d_count = nullptr;
	if (coverage) {
		const size_t bins = (size_t)first_small * n * 256; // of levels 1 .. first_small; the tail keeps its bins in LDS
		Grow grow{ctx};
		if (int rc = grow(tc->d_hist, bins + 1)) return rc;
		if (grow.drained) tc->images_in_flight = false;
		LMX_HIP(ctx, hipMemsetAsync(tc->d_hist.p, 0, (bins + 1) * sizeof(uint32_t), ctx->stream));
		d_count = tc->d_hist.p + bins;
		LMX_HIP(ctx, launch_mip_coverage(ctx->stream, tc->d_own.p, w * h, tm_coverage_ref(options->scale_coverage_ref), d_count)); // image (face 0, slice 0, mip 0) alone
	}
	uint32_t at = 0;
	for (uint32_t m = 1; m <= first_small; ++m) {
		TmLevel L;
		L.chains = tc->d_own.p;
		L.n_images = n;
		L.chain_px = chain_px;
		L.src_at = at;
		L.w = tm_side(w, m - 1);
		L.h = tm_side(h, m - 1);
		at += L.w * L.h;
		L.dst_at = at;
		L.dst_w = tm_side(w, m);
		L.dst_h = tm_side(h, m);
		L.rows_x = tc->d_rows.p + tc->rows_at[m];
		L.rows_y = L.rows_x + L.dst_w;
		L.tables = tc->d_mip_tables.p;
		L.histogram = coverage ? tc->d_hist.p + (size_t)(m - 1) * n * 256 : nullptr;
		LMX_HIP(ctx, launch_mip_level(ctx->stream, options->mode, L, tc->windows[2 * m], tc->windows[2 * m + 1]));
		// the scaled level is what the next one is computed from; level 0 is never scaled
		if (coverage) LMX_HIP(ctx, launch_mip_scale(ctx->stream, tc->d_own.p, n, chain_px, L.dst_at, L.dst_w * L.dst_h, L.histogram, d_count, w * h, options->scale_coverage_ref));
	}
	if (first_small + 1 < levels) {
		TmTail T;
		T.chains = tc->d_own.p;
		T.n_images = n;
		T.chain_px = chain_px;
		T.at = at;
		T.w = tm_side(w, first_small);
		T.h = tm_side(h, first_small);
		T.rows = tc->d_rows.p + tc->rows_at[first_small + 1];
		T.tables = tc->d_mip_tables.p;
		T.count = d_count;
		T.count_pixels = w * h;
		T.ref_norm = options->scale_coverage_ref;
		LMX_HIP(ctx, launch_mip_tail(ctx->stream, options->mode, T));
	}
	tc->mips_done = true;
	return LMX_OK;
}

int lmx_texcomp_read_pixels(LmxTexCompressor* tc, uint8_t* out, uint64_t cap_bytes) {
	LMX_ENTER(tc);
	if (!tc->chains || !tc->mips_done) return fail(ctx, LMX_ERR_NOT_BUILT, "texcomp: read_pixels before set_chains and generate_mips");
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	const size_t used = 4 * (size_t)tm_chain_pixels(tc->chain_w, tc->chain_h) * tc->chain_n;
	const int rc = read_out(ctx, out, (size_t)cap_bytes, reinterpret_cast<const uint8_t*>(tc->d_own.p), used, used + 4 * TC_GUARD_WORDS, "bytes of pixels");
	if (rc == LMX_OK) tc->images_in_flight = false; // (the read drained the stream)
	return rc;
}

int lmx_texmips_coeffs(uint32_t in, uint32_t out, void* rows, uint32_t cap_rows) {
	if (!rows || in == 0 || out == 0 || out > in) return LMX_ERR_INVALID_ARGUMENT;
	if (cap_rows < out) return LMX_ERR_CAPACITY;
	std::vector<TmRow> r;
	try {
		r.resize(out);
	} catch (const std::bad_alloc&) {
		return LMX_ERR_OUT_OF_MEMORY;
	}
	if (!tm_build_coeffs(in, out, r.data())) return LMX_ERR_UNSUPPORTED;
	memcpy(rows, r.data(), (size_t)out * sizeof(TmRow)); // (the caller's array need not be aligned)
	return LMX_OK;
}

int lmx_texmips_host(const LmxTexMipOptions* options, uint32_t n, uint32_t w, uint32_t h, const uint8_t* rgba, uint8_t* out) {
	if (!options || !mode_ok(options->mode) || !rgba || !out) return LMX_ERR_INVALID_ARGUMENT;
	uint64_t pixels;
	const char* what;
	if (int rc = chains_lay_out(n, w, h, &pixels, &what)) return rc;
	if (options->mode == LMX_TEXMIP_STOCHASTIC && (w > TM_STOCHASTIC_MAX_SIDE || h > TM_STOCHASTIC_MAX_SIDE)) return LMX_ERR_CAPACITY;
	const uint32_t levels = tm_levels(w, h);
	const size_t chain_px = (size_t)tm_chain_pixels(w, h);
	std::vector<TmRow> rows;
	std::vector<uint32_t> rows_at, windows, chain;
	std::vector<TmPx> scratch;
	TmTables tables;
	tm_build_tables(&tables);
	try {
		if (!chain_rows(w, h, &rows, &rows_at, &windows)) return LMX_ERR_UNSUPPORTED;
		chain.resize(chain_px);
		scratch.resize((size_t)h * tm_side(w, 1));
	} catch (const std::bad_alloc&) {
		return LMX_ERR_OUT_OF_MEMORY;
	}
	const bool coverage = options->scale_coverage_ref >= 0.0f;
	float wanted = -1;
	if (coverage) {
		const uint32_t ref = tm_coverage_ref(options->scale_coverage_ref);
		uint32_t count = 0;
		for (size_t i = 0; i < (size_t)w * h; ++i) count += rgba[4 * i + 3] > ref ? 1u : 0u;
		wanted = tm_coverage(count, w * h);
	}
	for (uint32_t i = 0; i < n; ++i) {
		memcpy(chain.data(), rgba + 4 * (size_t)w * h * i, 4 * (size_t)w * h);
		size_t at = 0;
		for (uint32_t m = 1; m < levels; ++m) {
			const uint32_t sw = tm_side(w, m - 1), sh = tm_side(h, m - 1), dw = tm_side(w, m), dh = tm_side(h, m);
			uint32_t* dst = chain.data() + at + (size_t)sw * sh;
			const TmRow* rx = rows.data() + rows_at[m];
			tm_level_host(options->mode, chain.data() + at, sw, sh, dst, dw, dh, rx, rx + dw, tables, scratch.data());
			if (coverage) {
				uint32_t histogram[256] = {};
				for (uint32_t k = 0; k < dw * dh; ++k) ++histogram[dst[k] >> 24];
				const float scale = tm_coverage_scale(histogram, dw * dh, options->scale_coverage_ref, wanted);
				for (uint32_t k = 0; k < dw * dh; ++k) dst[k] = tm_scale_alpha(dst[k], scale);
			}
			at += (size_t)sw * sh;
		}
		memcpy(out + 4 * chain_px * i, chain.data(), 4 * chain_px);
	}
	return LMX_OK;
}

} // extern "C"
