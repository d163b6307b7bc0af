// lmx_capi_animcomp.hip — the animation compressor's entry points (include/lumix_mi355.h, "Animation compressor"): what
// ModelImporter::writeAnimations (renderer/editor/model_importer.cpp:1508-1754) does per clip, per bone, per sample, for a batch of clips, as an
// object beside the context. The host side lays the batch out and launches animcomp_kernels.hip; the arithmetic is lmx_animcomp.h's.
#include "lmx_context.h"
#include "lmx_animcomp.h"

#include <new>

using namespace lmx;

struct LmxAnimCompressor {
	LmxContext* ctx = nullptr;
	uint32_t n_clips = 0, n_bones = 0; // the batch of the last set
	bool ran = false;
	uint64_t n_records = 0;            // of keys
	std::vector<AcClip> h_clips;
	std::vector<AcRangeItem> h_range_items;
	std::vector<AcPackItem> h_pack_items;
	std::vector<uint8_t> h_has_keys;
	std::vector<float> h_bind, h_fps;
	std::vector<LmxAnimCompInfo> h_infos;                // read once per run
	std::vector<uint64_t> t_word_at, r_word_at;          // per clip: where its streams start, in dwords
	uint64_t t_words = 0, r_words = 0, n_partials = 0;
	const float* d_keys = nullptr;                       // d_own.p or the caller's
	DevBuf<float> d_own, d_bind;
	DevBuf<uint8_t> d_has_keys;
	DevBuf<AcClip> d_clips;
	DevBuf<AcRangeItem> d_range_items;
	DevBuf<AcPackItem> d_pack_items;
	DevBuf<AcRange> d_partials;
	DevBuf<LmxAnimCompInfo> d_infos;
	DevBuf<LmxAnimConstTranslation> d_ct;
	DevBuf<LmxAnimTranslationTrack> d_tt;
	DevBuf<LmxAnimConstRotation> d_cr;
	DevBuf<LmxAnimRotationTrack> d_rt;
	DevBuf<AcTrack> d_t_tracks, d_r_tracks;
	DevBuf<uint32_t> d_t_stream, d_r_stream;
};

namespace {

constexpr size_t AC_GUARD_WORDS = 64; // behind the streams of a run: filled, never written by a kernel (lmx_context.h, fill_guard)

// the batch's layout from its descriptors; `what`: what was wrong, for the message
int lay_out(uint32_t n, const LmxAnimCompClip* descs, LmxAnimCompressor* ac, const char** what) {
	*what = "";
	if (n == 0 || !descs) {
		*what = "an empty batch or null descriptors";
		return LMX_ERR_INVALID_ARGUMENT;
	}
	uint64_t bones = 0, records = 0, partials = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const LmxAnimCompClip& d = descs[i];
		if (d.n_bones == 0 || d.n_bones > LMX_MAX_BONES) {
			*what = "a clip without bones or with more than LMX_MAX_BONES";
			return LMX_ERR_INVALID_ARGUMENT;
		}
		if (!d.bind_positions) {
			*what = "a clip without bind positions";
			return LMX_ERR_INVALID_ARGUMENT;
		}
		constexpr uint64_t cap = LMX_ANIMCOMP_MAX_BATCH_BYTES / sizeof(LmxAnimKey);
		const uint64_t own = (uint64_t)d.n_bones * d.n_samples;
		if (d.key_offset > cap || own > cap || d.key_offset + own > cap) {
			*what = "keys above LMX_ANIMCOMP_MAX_BATCH_BYTES";
			return LMX_ERR_CAPACITY;
		}
		records = std::max(records, d.key_offset + own);
		bones += d.n_bones;
		partials += (uint64_t)((d.n_samples + AC_RANGE_SAMPLES - 1) / AC_RANGE_SAMPLES) * d.n_bones * 7; // (at most a 64th of the keys' floats)
		if (bones > 0x7fffffffull || partials > 0x7fffffffull) {
			*what = "more bones in one batch than the tables' 32-bit offsets hold";
			return LMX_ERR_CAPACITY;
		}
	}
	try {
		ac->h_clips.resize(n);
		ac->h_has_keys.assign((size_t)bones, 1);
		ac->h_bind.resize(3 * (size_t)bones);
		ac->h_range_items.clear();
		uint32_t bone_off = 0, part_off = 0;
		for (uint32_t i = 0; i < n; ++i) {
			const LmxAnimCompClip& d = descs[i];
			ac->h_clips[i] = AcClip{d.n_bones, d.n_samples, bone_off, part_off, d.key_offset, d.translation_error, d.rotation_error};
			if (d.has_keys) memcpy(ac->h_has_keys.data() + bone_off, d.has_keys, d.n_bones);
			memcpy(ac->h_bind.data() + 3 * (size_t)bone_off, d.bind_positions, 12 * (size_t)d.n_bones);
			const uint32_t chunks = (d.n_samples + AC_RANGE_SAMPLES - 1) / AC_RANGE_SAMPLES;
			for (uint32_t k = 0; k < chunks; ++k) ac->h_range_items.push_back(AcRangeItem{i, k});
			bone_off += d.n_bones;
			part_off += chunks * d.n_bones * 7;
		}
		ac->h_fps.resize(n);
		for (uint32_t i = 0; i < n; ++i) ac->h_fps[i] = descs[i].fps;
		ac->h_infos.assign(n, LmxAnimCompInfo{});
		ac->t_word_at.assign(n, 0);
		ac->r_word_at.assign(n, 0);
	} catch (const std::bad_alloc&) {
		*what = "host allocation of the batch's tables failed";
		return LMX_ERR_OUT_OF_MEMORY;
	}
	ac->n_records = records;
	ac->n_partials = partials;
	ac->n_bones = (uint32_t)bones;
	return LMX_OK;
}

int set_clips(LmxAnimCompressor* ac, uint32_t n, const LmxAnimCompClip* descs, const LmxAnimKey* keys, bool on_device) {
	LmxContext* ctx = ac->ctx;
	if (n && descs && !keys) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: null keys");
	if (on_device && ((uintptr_t)keys & 3u)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: device keys are read as 32-bit words: the pointer must be a multiple of 4");
	// the tables of the set before may still be read by queued kernels or on-stream copies
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	ac->n_clips = 0;
	ac->ran = false;
	ac->d_keys = nullptr;
	const char* what;
	if (int rc = lay_out(n, descs, ac, &what)) return fail(ctx, rc, "animcomp: %s", what);
	const size_t bones = ac->n_bones;
	LMX_HIP(ctx, upload_on_stream(ac->d_clips, ac->h_clips, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ac->d_range_items, ac->h_range_items, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ac->d_has_keys, ac->h_has_keys, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ac->d_bind, ac->h_bind, ctx->stream));
	LMX_HIP(ctx, ac->d_partials.reserve(std::max<size_t>((size_t)ac->n_partials, 1)));
	LMX_HIP(ctx, ac->d_infos.reserve(n));
	LMX_HIP(ctx, ac->d_ct.reserve(bones));
	LMX_HIP(ctx, ac->d_tt.reserve(bones));
	LMX_HIP(ctx, ac->d_cr.reserve(bones));
	LMX_HIP(ctx, ac->d_rt.reserve(bones));
	LMX_HIP(ctx, ac->d_t_tracks.reserve(bones));
	LMX_HIP(ctx, ac->d_r_tracks.reserve(bones));
	if (on_device) ac->d_keys = reinterpret_cast<const float*>(keys);
	else {
		LMX_HIP(ctx, upload_on_stream(ac->d_own, reinterpret_cast<const float*>(keys), 7 * (size_t)ac->n_records, ctx->stream));
		ac->d_keys = ac->d_own.p;
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's arrays have been read when this returns)
	ac->n_clips = n;
	return LMX_OK;
}

AcBatch batch_of(const LmxAnimCompressor* ac) {
	AcBatch b;
	b.clips = ac->d_clips.p, b.keys = ac->d_keys, b.has_keys = ac->d_has_keys.p, b.bind = ac->d_bind.p, b.partials = ac->d_partials.p, b.infos = ac->d_infos.p;
	b.ct = ac->d_ct.p, b.tt = ac->d_tt.p, b.cr = ac->d_cr.p, b.rt = ac->d_rt.p, b.t_tracks = ac->d_t_tracks.p, b.r_tracks = ac->d_r_tracks.p;
	return b;
}

} // namespace

namespace lmx {

int animcomp_clip_view(LmxContext* ctx, LmxAnimCompressor* ac, uint32_t clip, AnimCompClipView* out) {
	if (ac->ctx != ctx) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: the compressor belongs to another context");
	if (!ac->ran) return fail(ctx, LMX_ERR_NOT_BUILT, "animcomp: no run on this batch");
	if (clip >= ac->n_clips) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: clip %u of %u", clip, ac->n_clips);
	const LmxAnimCompInfo& info = ac->h_infos[clip];
	if (info.status) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: clip %u was refused with status %u", clip, info.status);
	try {
		out->ct.resize(info.n_const_translations), out->tt.resize(info.n_translations), out->cr.resize(info.n_const_rotations), out->rt.resize(info.n_rotations);
	} catch (const std::bad_alloc&) {
		return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "animcomp: host allocation of the clip's tables failed");
	}
	const uint32_t at = ac->h_clips[clip].bone_off;
	LMX_HIP(ctx, read_back(out->ct.data(), (const LmxAnimConstTranslation*)ac->d_ct.p + at, out->ct.size(), ctx->stream));
	LMX_HIP(ctx, read_back(out->tt.data(), (const LmxAnimTranslationTrack*)ac->d_tt.p + at, out->tt.size(), ctx->stream));
	LMX_HIP(ctx, read_back(out->cr.data(), (const LmxAnimConstRotation*)ac->d_cr.p + at, out->cr.size(), ctx->stream));
	LMX_HIP(ctx, read_back(out->rt.data(), (const LmxAnimRotationTrack*)ac->d_rt.p + at, out->rt.size(), ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	out->info = info;
	out->fps = ac->h_fps[clip];
	out->d_translation_stream = reinterpret_cast<const uint8_t*>(ac->d_t_stream.p + ac->t_word_at[clip]);
	out->d_rotation_stream = reinterpret_cast<const uint8_t*>(ac->d_r_stream.p + ac->r_word_at[clip]);
	return LMX_OK;
}

} // namespace lmx

extern "C" {

int lmx_animcomp_create(LmxContext* ctx, LmxAnimCompressor** out) { return object_create(ctx, out, "animcomp"); }

void lmx_animcomp_destroy(LmxAnimCompressor* ac) {
	if (ac) object_destroy(ac);
}

int lmx_animcomp_set_clips(LmxAnimCompressor* ac, uint32_t n, const LmxAnimCompClip* descs, const LmxAnimKey* keys) {
	LMX_ENTER(ac);
	return set_clips(ac, n, descs, keys, false);
}

int lmx_animcomp_set_clips_device(LmxAnimCompressor* ac, uint32_t n, const LmxAnimCompClip* descs, const LmxAnimKey* d_keys) {
	LMX_ENTER(ac);
	return set_clips(ac, n, descs, d_keys, true);
}

int lmx_animcomp_run(LmxAnimCompressor* ac) {
	LMX_ENTER(ac);
	if (!ac->n_clips || !ac->d_keys) return fail(ctx, LMX_ERR_NOT_BUILT, "animcomp: run before a batch was set");
	const uint32_t n = ac->n_clips;
	ac->ran = false;
	const AcBatch batch = batch_of(ac);
	LMX_HIP(ctx, launch_animcomp_ranges(ctx->stream, batch, ac->d_range_items.p, (uint32_t)ac->h_range_items.size()));
	LMX_HIP(ctx, launch_animcomp_layout(ctx->stream, batch, n));
	// the run's one host wait: the frame sizes size the streams and the pack's grid
	if (int rc = read_now(ctx, ac->h_infos.data(), (const LmxAnimCompInfo*)ac->d_infos.p, (size_t)n)) return rc;
	uint64_t t_words = 0, r_words = 0;
	try {
		ac->h_pack_items.clear();
		for (uint32_t i = 0; i < n; ++i) {
			const LmxAnimCompInfo& info = ac->h_infos[i];
			ac->t_word_at[i] = t_words;
			ac->r_word_at[i] = r_words;
			if (info.status) continue;
			const uint32_t groups = (ac->h_clips[i].n_samples + AC_GROUP_FRAMES - 1) / AC_GROUP_FRAMES;
			for (uint32_t rotation = 0; rotation < 2; ++rotation) {
				const uint32_t tracks = rotation ? info.n_rotations : info.n_translations;
				if (!tracks) continue;
				const uint32_t per = std::max<uint32_t>(1u, AC_PACK_ENTRIES / (AC_GROUP_FRAMES * tracks));
				for (uint32_t g = 0; g < groups; g += per) ac->h_pack_items.push_back(AcPackItem{i, rotation, g, std::min(per, groups - g), (uint32_t)(rotation ? r_words : t_words), 0u});
			}
			t_words += (info.translation_stream_size + 3) / 4;
			r_words += (info.rotation_stream_size + 3) / 4;
		}
	} catch (const std::bad_alloc&) {
		return fail(ctx, LMX_ERR_OUT_OF_MEMORY, "animcomp: host allocation of the pack's work list failed");
	}
	if (t_words > 0xffffffffull || r_words > 0xffffffffull) return fail(ctx, LMX_ERR_CAPACITY, "animcomp: the streams of this batch pass 2^32 dwords");
	// (the stream has drained: nothing reads the buffers a reserve frees)
	LMX_HIP(ctx, ac->d_t_stream.reserve((size_t)t_words + AC_GUARD_WORDS));
	LMX_HIP(ctx, ac->d_r_stream.reserve((size_t)r_words + AC_GUARD_WORDS));
	LMX_HIP(ctx, fill_guard(ac->d_t_stream.p + t_words, AC_GUARD_WORDS, ctx->stream));
	LMX_HIP(ctx, fill_guard(ac->d_r_stream.p + r_words, AC_GUARD_WORDS, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(ac->d_pack_items, ac->h_pack_items, ctx->stream)); // (h_pack_items stays until the next run, which waits first)
	LMX_HIP(ctx, launch_animcomp_pack(ctx->stream, batch, ac->d_pack_items.p, (uint32_t)ac->h_pack_items.size(), ac->d_t_stream.p, ac->d_r_stream.p));
	ac->t_words = t_words;
	ac->r_words = r_words;
	ac->ran = true;
	return LMX_OK;
}

int lmx_animcomp_clip_info(LmxAnimCompressor* ac, uint32_t clip, LmxAnimCompInfo* out) {
	LMX_ENTER(ac);
	if (!ac->ran) return fail(ctx, LMX_ERR_NOT_BUILT, "animcomp: no run on this batch");
	if (!out || clip >= ac->n_clips) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: null out, or clip %u of %u", clip, ac->n_clips);
	*out = ac->h_infos[clip];
	return LMX_OK;
}

int lmx_animcomp_read_clip(LmxAnimCompressor* ac, uint32_t clip, LmxAnimCompOutput* out) {
	LMX_ENTER(ac);
	if (!ac->ran) return fail(ctx, LMX_ERR_NOT_BUILT, "animcomp: no run on this batch");
	if (!out || clip >= ac->n_clips) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: null out, or clip %u of %u", clip, ac->n_clips);
	const LmxAnimCompInfo& info = ac->h_infos[clip];
	if (info.status) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "animcomp: clip %u was refused with status %u", clip, info.status);
	const uint32_t most = std::max(std::max(info.n_const_translations, info.n_translations), std::max(info.n_const_rotations, info.n_rotations));
	if (out->cap_tracks < most) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u track records in each table", most);
	if (out->cap_translation_stream < info.translation_stream_size || out->cap_rotation_stream < info.rotation_stream_size)
		return fail(ctx, LMX_ERR_CAPACITY, "need room for %llu / %llu bytes of streams", (unsigned long long)info.translation_stream_size, (unsigned long long)info.rotation_stream_size);
	const uint32_t at = ac->h_clips[clip].bone_off;
	LMX_HIP(ctx, read_back(out->const_translations, (const LmxAnimConstTranslation*)ac->d_ct.p + at, info.n_const_translations, ctx->stream));
	LMX_HIP(ctx, read_back(out->translations, (const LmxAnimTranslationTrack*)ac->d_tt.p + at, info.n_translations, ctx->stream));
	LMX_HIP(ctx, read_back(out->const_rotations, (const LmxAnimConstRotation*)ac->d_cr.p + at, info.n_const_rotations, ctx->stream));
	LMX_HIP(ctx, read_back(out->rotations, (const LmxAnimRotationTrack*)ac->d_rt.p + at, info.n_rotations, ctx->stream));
	LMX_HIP(ctx, read_back(out->translation_stream, reinterpret_cast<const uint8_t*>(ac->d_t_stream.p + ac->t_word_at[clip]), (size_t)info.translation_stream_size, ctx->stream));
	LMX_HIP(ctx, read_back(out->rotation_stream, reinterpret_cast<const uint8_t*>(ac->d_r_stream.p + ac->r_word_at[clip]), (size_t)info.rotation_stream_size, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return LMX_OK;
}

int lmx_animcomp_device_outputs(LmxAnimCompressor* ac, LmxAnimCompDevice* out, uint32_t* bone_offset, uint64_t* translation_offset, uint64_t* rotation_offset) {
	LMX_ENTER(ac);
	if (!out) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null out");
	if (!ac->n_clips) return fail(ctx, LMX_ERR_NOT_BUILT, "animcomp: no batch");
	memset(out, 0, sizeof(*out));
	out->d_keys = reinterpret_cast<const LmxAnimKey*>(ac->d_keys);
	if (ac->ran) {
		out->d_infos = ac->d_infos.p;
		out->d_const_translations = ac->d_ct.p, out->d_translations = ac->d_tt.p, out->d_const_rotations = ac->d_cr.p, out->d_rotations = ac->d_rt.p;
		out->d_translation_streams = reinterpret_cast<const uint8_t*>(ac->d_t_stream.p);
		out->d_rotation_streams = reinterpret_cast<const uint8_t*>(ac->d_r_stream.p);
	}
	out->n_clips = ac->n_clips;
	out->n_bones = ac->n_bones;
	for (uint32_t i = 0; i < ac->n_clips; ++i) {
		if (bone_offset) bone_offset[i] = ac->h_clips[i].bone_off;
		if (translation_offset) translation_offset[i] = 4 * ac->t_word_at[i];
		if (rotation_offset) rotation_offset[i] = 4 * ac->r_word_at[i];
	}
	return LMX_OK;
}

int lmx_animcomp_compress_host(const LmxAnimCompClip* desc, const LmxAnimKey* keys, LmxAnimCompInfo* info, LmxAnimCompOutput* out) {
	if (!desc || !info || desc->n_bones == 0 || desc->n_bones > LMX_MAX_BONES || !desc->bind_positions || (!keys && desc->n_samples)) return LMX_ERR_INVALID_ARGUMENT;
	return ac_compress_host(*desc, reinterpret_cast<const float*>(keys), info, out) ? LMX_OK : LMX_ERR_CAPACITY;
}

} // extern "C"
