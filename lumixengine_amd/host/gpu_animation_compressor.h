// gpu_animation_compressor.h — the animation compressor's host adapter (C++ host side of include/lumix_mi355.h "Animation compressor").
//
// In the reference ModelImporter::writeAnimations' write_animation (src/renderer/editor/model_importer.cpp:1519-1743) writes one .ani file
// per clip: the header, the skeleton path, fps, samples - 1 and the root-motion flags, then from all_keys the translation tracks and their
// bit stream and the rotation tracks and theirs - per clip, per bone, per sample on one thread. GpuAnimationCompressor::compress writes the
// same bytes with those loops on the device:
//   - the keys are transposed from the importer's Array<Array<Key>> (per bone, per sample; an empty array: a bone without keys) to the
//     ABI's records, sample-major and bones-minor;
//   - one lmx_animcomp_run for all clips handed over, one read per clip;
//   - per clip the file as write_animation lays it out: Animation::Header, the skeleton path and its zero, fps, samples - 1, flags, the
//     translation count, its records in bone order - constant and animated ones interleaved as the bones come: name hash, TrackType, then
//     the value, or min, to_range, bitsizes and offset_bits - and the translation stream; the rotation count, its records (an animated one:
//     the three kept channels' min, to_range and bit sizes, offset_bits, skipped_channel) and the rotation stream.
// What stays with the importer: fillTracks and the FBX curves behind it (the keys come sampled), the bind position of each bone relative to
// its parent, baking root motion at load, and writing the file.
// A clip the library refuses (lastStatus() says with what: LMX_ANIMCOMP_*) returns false and leaves `dst` as it was.
//
// `KeysT` is Array<Array<ModelImporter::Key>>-shaped (size(), operator[] -> an array with size(), empty() and operator[] -> {pos, rot}),
// `StreamT` OutputMemoryStream-shaped (write(ptr, bytes), size(), resize(bytes)). Animation::Header, Animation::TrackType, Animation::Version
// and BoneNameHash are the engine's inside it (-DLMX_WITH_LUMIX_HEADERS); a standalone build takes them from
// tests/cpp/lumix_compat_animcomp.h.
#pragma once

#include <string.h>

#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "animation/animation.h"
	#include "core/hash.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_animcomp.h"
#endif

namespace Lumix {

struct GpuAnimationCompressor {
	// one clip as write_animation sees it
	template <typename KeysT> struct Clip {
		const KeysT* all_keys;          // per bone: its samples, or none
		u32 samples_count;
		float fps;
		u32 root_motion_flags;          // ModelMeta::root_motion_flags
		float translation_error = 1.f;  // ModelMeta::anim_translation_error
		float rotation_error = 1.f;     // ModelMeta::anim_rotation_error
	};

	explicit GpuAnimationCompressor(LmxContext* ctx) : m_ctx(ctx) { lmx_animcomp_create(ctx, &m_ac); }
	~GpuAnimationCompressor() { lmx_animcomp_destroy(m_ac); }
	GpuAnimationCompressor(const GpuAnimationCompressor&) = delete;
	void operator=(const GpuAnimationCompressor&) = delete;

	// the skeleton all clips of a batch share: each bone's local bind position (what :1549-1556 computes) and its name hash
	void setSkeleton(const Vec3* bind_positions, const BoneNameHash* bone_hashes, u32 n_bones, const char* skeleton_path) {
		m_bind.resize(3 * (size_t)n_bones);
		for (u32 b = 0; b < n_bones; ++b) m_bind[3 * b] = bind_positions[b].x, m_bind[3 * b + 1] = bind_positions[b].y, m_bind[3 * b + 2] = bind_positions[b].z;
		m_hashes.assign(bone_hashes, bone_hashes + n_bones);
		m_path.assign(skeleton_path, skeleton_path + strlen(skeleton_path) + 1); // writeString: the characters and a zero
	}

	// the device work of a batch of clips: true when the batch ran (single clips may still be refused: write() says)
	template <typename KeysT> bool compress(const Clip<KeysT>* clips, u32 n_clips) {
		m_ran = 0;
		m_status = 0;
		const u32 nb = (u32)m_hashes.size();
		if (!m_ac || !n_clips || !nb) return false;
		m_descs.resize(n_clips);
		m_has.assign((size_t)n_clips * nb, 0);
		size_t records = 0;
		for (u32 i = 0; i < n_clips; ++i) {
			if ((u32)clips[i].all_keys->size() != nb) return false;
			records += (size_t)clips[i].samples_count * nb;
		}
		m_keys.resize(records);
		m_clips.resize(n_clips);
		size_t at = 0;
		for (u32 i = 0; i < n_clips; ++i) {
			const KeysT& all_keys = *clips[i].all_keys;
			const u32 ns = clips[i].samples_count;
			for (u32 b = 0; b < nb; ++b) {
				const auto& keys = all_keys[b];
				if (keys.empty()) { // (its records stay zeros: nothing reads them)
					for (u32 s = 0; s < ns; ++s) m_keys[at + (size_t)s * nb + b] = LmxAnimKey{{0, 0, 0}, {0, 0, 0, 1}};
					continue;
				}
				if ((u32)keys.size() < ns) return false;
				m_has[(size_t)i * nb + b] = 1;
				for (u32 s = 0; s < ns; ++s) {
					const auto& k = keys[s];
					m_keys[at + (size_t)s * nb + b] = LmxAnimKey{{k.pos.x, k.pos.y, k.pos.z}, {k.rot.x, k.rot.y, k.rot.z, k.rot.w}};
				}
			}
			LmxAnimCompClip& d = m_descs[i];
			memset(&d, 0, sizeof(d));
			d.n_bones = nb, d.n_samples = ns, d.fps = clips[i].fps;
			d.translation_error = clips[i].translation_error, d.rotation_error = clips[i].rotation_error;
			d.has_keys = m_has.data() + (size_t)i * nb, d.bind_positions = m_bind.data(), d.key_offset = at;
			m_clips[i] = Meta{clips[i].fps, ns, clips[i].root_motion_flags};
			at += (size_t)ns * nb;
		}
		if (lmx_animcomp_set_clips(m_ac, n_clips, m_descs.data(), m_keys.empty() ? &m_no_key : m_keys.data()) != LMX_OK) return false;
		if (lmx_animcomp_run(m_ac) != LMX_OK) return false;
		m_ran = n_clips;
		return true;
	}

	// clip `i` of the last compress(): the .ani bytes appended to `dst`
	template <typename StreamT> bool write(u32 i, StreamT& dst) {
		if (i >= m_ran) return false;
		LmxAnimCompInfo info;
		if (lmx_animcomp_clip_info(m_ac, i, &info) != LMX_OK) return false;
		m_status = info.status;
		if (info.status) return false;
		const u32 most = maximum(maximum(info.n_const_translations, info.n_translations), maximum(info.n_const_rotations, info.n_rotations));
		m_ct.resize(most), m_tt.resize(most), m_cr.resize(most), m_rt.resize(most);
		m_ts.resize((size_t)info.translation_stream_size), m_rs.resize((size_t)info.rotation_stream_size);
		LmxAnimCompOutput out;
		memset(&out, 0, sizeof(out));
		out.const_translations = m_ct.data(), out.translations = m_tt.data(), out.const_rotations = m_cr.data(), out.rotations = m_rt.data();
		out.translation_stream = m_ts.data(), out.rotation_stream = m_rs.data();
		out.cap_tracks = most, out.cap_translation_stream = m_ts.size(), out.cap_rotation_stream = m_rs.size();
		if (lmx_animcomp_read_clip(m_ac, i, &out) != LMX_OK) return false;
		Animation::Header header; // :1521-1524
		header.magic = Animation::HEADER_MAGIC;
		header.version = Animation::Version::LAST;
		put(dst, header);
		dst.write(m_path.data(), m_path.size());
		put(dst, m_clips[i].fps);
		put(dst, (u32)(m_clips[i].samples - 1));
		put(dst, m_clips[i].flags);
		// the two kinds of record in one list, as the bones come (:1544-1605): both tables are in bone order, so this is a merge
		put(dst, (u32)(info.n_const_translations + info.n_translations));
		for (u32 c = 0, a = 0; c < info.n_const_translations || a < info.n_translations;) {
			if (a == info.n_translations || (c < info.n_const_translations && m_ct[c].bone_index < m_tt[a].bone_index)) {
				put(dst, m_hashes[m_ct[c].bone_index]);
				put(dst, Animation::TrackType::CONSTANT);
				dst.write(m_ct[c].value, sizeof(m_ct[c].value));
				++c;
			} else {
				const LmxAnimTranslationTrack& t = m_tt[a++];
				put(dst, m_hashes[t.bone_index]);
				put(dst, Animation::TrackType::ANIMATED);
				dst.write(t.min, sizeof(t.min));
				dst.write(t.to_range, sizeof(t.to_range));
				dst.write(t.bitsizes, sizeof(t.bitsizes));
				put(dst, t.offset_bits);
			}
		}
		dst.write(m_ts.data(), m_ts.size());
		put(dst, (u32)(info.n_const_rotations + info.n_rotations)); // :1628-1714
		for (u32 c = 0, a = 0; c < info.n_const_rotations || a < info.n_rotations;) {
			if (a == info.n_rotations || (c < info.n_const_rotations && m_cr[c].bone_index < m_rt[a].bone_index)) {
				put(dst, m_hashes[m_cr[c].bone_index]);
				put(dst, Animation::TrackType::CONSTANT);
				dst.write(m_cr[c].value, sizeof(m_cr[c].value));
				++c;
			} else {
				const LmxAnimRotationTrack& t = m_rt[a++];
				put(dst, m_hashes[t.bone_index]);
				put(dst, Animation::TrackType::ANIMATED);
				dst.write(t.min, sizeof(t.min));
				dst.write(t.to_range, sizeof(t.to_range));
				dst.write(t.bitsizes, sizeof(t.bitsizes));
				put(dst, t.offset_bits);
				put(dst, t.skipped_channel);
			}
		}
		dst.write(m_rs.data(), m_rs.size());
		return true;
	}

	u32 lastStatus() const { return m_status; } // of the clip the last write() refused: LMX_ANIMCOMP_*
	const char* lastError() const { return lmx_last_error(m_ctx); }
	LmxAnimCompressor* handle() const { return m_ac; }

private:
	struct Meta {
		float fps;
		u32 samples, flags;
	};
	template <typename StreamT, typename T> static void put(StreamT& dst, const T& v) { dst.write(&v, sizeof(v)); }
	static u32 maximum(u32 a, u32 b) { return a > b ? a : b; }

	LmxContext* m_ctx;
	LmxAnimCompressor* m_ac = nullptr;
	u32 m_ran = 0, m_status = 0;
	LmxAnimKey m_no_key = {};
	std::vector<float> m_bind;
	std::vector<BoneNameHash> m_hashes;
	std::vector<char> m_path;
	std::vector<LmxAnimCompClip> m_descs;
	std::vector<u8> m_has;
	std::vector<LmxAnimKey> m_keys;
	std::vector<Meta> m_clips;
	std::vector<LmxAnimConstTranslation> m_ct;
	std::vector<LmxAnimTranslationTrack> m_tt;
	std::vector<LmxAnimConstRotation> m_cr;
	std::vector<LmxAnimRotationTrack> m_rt;
	std::vector<u8> m_ts, m_rs;
};

} // namespace Lumix
