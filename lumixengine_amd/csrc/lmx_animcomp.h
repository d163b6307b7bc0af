// lmx_animcomp.h — the arithmetic of the animation clip writer (ModelImporter::writeAnimations, renderer/editor/model_importer.cpp:1508-1754,
// helpers :34-146), shared by animcomp_kernels.hip and the host side of lmx_capi_animcomp.hip: the ordered min / max fold, the bit size of a
// range, the rotation clamp, the skipped channel, to_range, the two packs and a bone's whole layout. Bit for bit the reference's where it is
// defined; where it is not: a zero-range channel packs 0, log2 of 0 is 0, and a clip the reference would overflow on is
// refused with an LMX_ANIMCOMP_* code. FMA-free (-ffp-contract=off); nothing here may be reassociated. The launchers are at the end.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "lmx_math.h"
#include "lmx_types.h"

namespace lmx {

constexpr float AC_TRANSLATION_STEP = 0.00005f, AC_ROTATION_STEP = 0.000001f; // :1570, :1663
constexpr float AC_BIND_ERROR = 0.00001f;                                     // isBindPosePositionTrack, :164
constexpr uint32_t AC_MAX_CHANNEL_BITS = 30, AC_MAX_ENTRY_BITS = 57, AC_MAX_FRAME_BITS = 65535;
constexpr uint32_t AC_OFF_BIND = 1, AC_NONFINITE = 2; // AcRange::flags

LMX_HD bool ac_finite(float v) { return fabsf(v) <= FLT_MAX; }

// one channel of one bone over a run of samples: the reference's `p < min ? p : min` fold, so the earlier sample stays on a tie (and with it
// the sign of a zero)
struct AcRange {
	float mn, mx;
	uint32_t flags;
};
LMX_HD AcRange ac_range_identity() { return AcRange{FLT_MAX, -FLT_MAX, 0u}; }
LMX_HD void ac_range_add(AcRange& r, float v) {
	r.mn = v < r.mn ? v : r.mn;
	r.mx = v > r.mx ? v : r.mx;
	if (!ac_finite(v)) r.flags |= AC_NONFINITE;
}
// ... of a position channel: the bind-pose test rides along
LMX_HD void ac_range_add_pos(AcRange& r, float v, float bind) {
	ac_range_add(r, v);
	if (fabsf(v - bind) > AC_BIND_ERROR) r.flags |= AC_OFF_BIND;
}
// `later` covers samples behind those of `r`
LMX_HD void ac_range_join(AcRange& r, const AcRange& later) {
	r.mn = later.mn < r.mn ? later.mn : r.mn;
	r.mx = later.mx > r.mx ? later.mx : r.mx;
	r.flags |= later.flags;
}

LMX_HD void ac_refuse(uint32_t& code, uint32_t with) { code = code == 0 || with < code ? with : code; }

// (u8)log2(u32((max - min) / step / error)): both divisions in fp32, left to right; 31 - clz for an argument >= 1, 0 for 0
LMX_HD uint32_t ac_range_bits(float mn, float mx, float step, float error, uint32_t& code) {
	const float q = (mx - mn) / step / error;
	if (!(q < 4294967296.f)) {
		ac_refuse(code, LMX_ANIMCOMP_QUOTIENT_RANGE);
		return 0;
	}
	uint32_t u = (uint32_t)q, bits = 0;
	while (u >>= 1) ++bits;
	return bits;
}

// clampBitsizes, :119-146 (called with a non-zero sum): zeros become 1; above 64 the sizes are decremented round-robin from channel 0
LMX_HD void ac_clamp_bits(uint32_t bits[4]) {
	uint32_t total = 0;
	for (int i = 0; i < 4; ++i) {
		if (bits[i] == 0) bits[i] = 1;
		total += bits[i];
	}
	while (total > 64) // (whole rounds over constant indices: the same order of decrements, and the sizes stay in registers)
		for (int i = 0; i < 4; ++i)
			if (total > 64 && bits[i] > 0) {
				--bits[i];
				--total;
			}
}
LMX_HD uint32_t ac_skipped_channel(const uint32_t bits[4]) { // the first of the largest, :1681-1684
	uint32_t s = 0, most = bits[0];
	for (uint32_t i = 1; i < 4; ++i)
		if (bits[i] > most) {
			most = bits[i];
			s = i;
		}
	return s;
}
LMX_HD float ac_to_range(float mn, float mx, uint32_t bits) { return (mx - mn) / (float)(int)((1u << bits) - 1u); } // fp32 by int, :1591

// pack(v, min, range, bitsize), :79-82: fp32 difference, fp64 divide, fp64 multiply, + 0.5. A zero range gives 0; the field never leaves its bits
LMX_HD uint64_t ac_pack_field(float v, float mn, float range, uint32_t bits) {
	if (range == 0.f) return 0;
	const double normalized = (double)(v - mn) / (double)range;
	const double scaled = normalized * (double)(int)((1u << bits) - 1u);
	return (uint64_t)(scaled + 0.5) & ((1ull << bits) - 1ull);
}

// an animated track as the pack reads it (device table, bone order)
struct AcTrack {
	float mn[4], range[4]; // range = max - min in fp32, what pack divides by
	uint8_t bits[4];
	uint16_t offset_bits;
	uint8_t skipped;       // rotation: the channel left out
	uint8_t entry_bits;
	uint32_t bone;
};

LMX_HD uint64_t ac_pack_translation(const float* pos, const AcTrack& t) { // :107-117: x in the low bits
	uint64_t res = ac_pack_field(pos[2], t.mn[2], t.range[2], t.bits[2]);
	res <<= t.bits[1];
	res |= ac_pack_field(pos[1], t.mn[1], t.range[1], t.bits[1]);
	res <<= t.bits[0];
	res |= ac_pack_field(pos[0], t.mn[0], t.range[0], t.bits[0]);
	return res;
}
LMX_HD uint64_t ac_pack_rotation(const float* rot, const AcTrack& t) { // :84-105 and :1730-1732: sign bit, then the kept channels upwards
	uint64_t res = 0;
#pragma unroll
	for (int c = 3; c >= 0; --c) {
		if ((uint32_t)c == t.skipped) continue;
		res <<= t.bits[c];
		res |= ac_pack_field(rot[c], t.mn[c], t.range[c], t.bits[c]);
	}
	return (res << 1) | (rot[t.skipped] < 0.f ? 1ull : 0ull);
}

// what a bone becomes, from the folds of its seven channels (pos xyz, rot xyzw)
constexpr uint32_t AC_NONE = 0, AC_CONST = 1, AC_ANIMATED = 2;
struct AcBone {
	uint32_t t_kind, r_kind; // AC_*
	uint32_t t_bits[3], r_bits[4];
	uint32_t skipped, t_entry, r_entry;
	uint32_t code;           // LMX_ANIMCOMP_*: what this bone refuses the clip with, or 0
};
LMX_HD AcBone ac_bone_layout(const AcRange r[7], const float bind[3], float t_error, float r_error) {
	AcBone b;
	b.t_kind = b.r_kind = AC_NONE;
	b.skipped = b.t_entry = b.r_entry = b.code = 0;
	for (int c = 0; c < 3; ++c) b.t_bits[c] = 0;
	for (int c = 0; c < 4; ++c) b.r_bits[c] = 0;
	if (!ac_finite(bind[0]) || !ac_finite(bind[1]) || !ac_finite(bind[2])) ac_refuse(b.code, LMX_ANIMCOMP_NONFINITE_BIND);
	uint32_t flags = 0;
	for (int c = 0; c < 7; ++c) flags |= r[c].flags;
	if (flags & AC_NONFINITE) ac_refuse(b.code, LMX_ANIMCOMP_NONFINITE_KEY);
	if (b.code) return b;
	if (flags & AC_OFF_BIND) { // :1558
		uint32_t sum = 0;
		for (int c = 0; c < 3; ++c) {
			b.t_bits[c] = ac_range_bits(r[c].mn, r[c].mx, AC_TRANSLATION_STEP, t_error, b.code);
			sum += b.t_bits[c];
		}
		if (sum == 0) b.t_kind = AC_CONST;
		else {
			b.t_kind = AC_ANIMATED;
			for (int c = 0; c < 3; ++c) {
				if (b.t_bits[c] == 0) b.t_bits[c] = 1;
				if (b.t_bits[c] > AC_MAX_CHANNEL_BITS) ac_refuse(b.code, LMX_ANIMCOMP_CHANNEL_BITS);
				b.t_entry += b.t_bits[c];
			}
			if (b.t_entry > AC_MAX_ENTRY_BITS) ac_refuse(b.code, LMX_ANIMCOMP_ENTRY_BITS);
		}
	}
	uint32_t sum = 0;
	for (int c = 0; c < 4; ++c) {
		b.r_bits[c] = ac_range_bits(r[3 + c].mn, r[3 + c].mx, AC_ROTATION_STEP, r_error, b.code);
		sum += b.r_bits[c];
	}
	if (sum == 0) b.r_kind = AC_CONST;
	else {
		b.r_kind = AC_ANIMATED;
		ac_clamp_bits(b.r_bits);
		b.skipped = ac_skipped_channel(b.r_bits);
		b.r_entry = 1;
		for (uint32_t c = 0; c < 4; ++c) {
			if (b.r_bits[c] > AC_MAX_CHANNEL_BITS) ac_refuse(b.code, LMX_ANIMCOMP_CHANNEL_BITS);
			if (c != b.skipped) b.r_entry += b.r_bits[c];
		}
		if (b.r_entry > AC_MAX_ENTRY_BITS) ac_refuse(b.code, LMX_ANIMCOMP_ENTRY_BITS);
	}
	return b;
}
// what refuses a clip before any bone is looked at
LMX_HD uint32_t ac_clip_code(uint32_t n_samples, float t_error, float r_error) {
	if (n_samples == 0) return LMX_ANIMCOMP_NO_SAMPLES;
	if (!ac_finite(t_error) || !ac_finite(r_error) || !(t_error > 0.f) || !(r_error > 0.f)) return LMX_ANIMCOMP_BAD_ERROR;
	return 0;
}

// the records of a bone, as the file and LmxAnimation hold them, and as the pack reads them
LMX_HD void ac_translation_records(const AcRange r[7], const AcBone& b, uint32_t bone, uint32_t offset_bits, LmxAnimTranslationTrack* rec, AcTrack* track) {
	memset(rec, 0, sizeof(*rec));
	memset(track, 0, sizeof(*track));
	for (int c = 0; c < 3; ++c) {
		rec->min[c] = track->mn[c] = r[c].mn;
		rec->to_range[c] = ac_to_range(r[c].mn, r[c].mx, b.t_bits[c]);
		rec->bitsizes[c] = track->bits[c] = (uint8_t)b.t_bits[c];
		track->range[c] = r[c].mx - r[c].mn;
	}
	rec->offset_bits = track->offset_bits = (uint16_t)offset_bits;
	rec->bone_index = (uint16_t)bone;
	track->bone = bone;
	track->skipped = 0xff;
	track->entry_bits = (uint8_t)b.t_entry;
}
LMX_HD void ac_rotation_records(const AcRange r[7], const AcBone& b, uint32_t bone, uint32_t offset_bits, LmxAnimRotationTrack* rec, AcTrack* track) {
	memset(rec, 0, sizeof(*rec));
	memset(track, 0, sizeof(*track));
	for (uint32_t c = 0; c < 4; ++c) {
		track->mn[c] = r[3 + c].mn;
		track->range[c] = r[3 + c].mx - r[3 + c].mn;
		track->bits[c] = (uint8_t)b.r_bits[c];
	}
	for (uint32_t k = 0; k < 3; ++k) { // the k-th kept channel is k, or k + 1 from the skipped one on (constant indices: registers on the device)
		const bool up = k >= b.skipped;
		const float mn = up ? r[4 + k].mn : r[3 + k].mn, mx = up ? r[4 + k].mx : r[3 + k].mx;
		const uint32_t bits = up ? b.r_bits[k + 1] : b.r_bits[k];
		rec->min[k] = mn;
		rec->to_range[k] = ac_to_range(mn, mx, bits);
		rec->bitsizes[k] = (uint8_t)bits;
	}
	rec->offset_bits = track->offset_bits = (uint16_t)offset_bits;
	rec->bone_index = (uint16_t)bone;
	rec->skipped_channel = track->skipped = (uint8_t)b.skipped;
	track->bone = bone;
	track->entry_bits = (uint8_t)b.r_entry;
}

// ---- a whole clip on the host, sample after sample like the reference --------------------------------------------------------------------------
// keys: the clip's n_samples x n_bones records of 7 floats. `out` may be null (the info alone); returns false where its arrays are too small.
inline bool ac_compress_host(const LmxAnimCompClip& d, const float* keys, LmxAnimCompInfo* info, LmxAnimCompOutput* out) {
	memset(info, 0, sizeof(*info));
	const uint32_t nb = d.n_bones, ns = d.n_samples;
	info->frame_count = ns ? ns - 1 : 0;
	info->status = ac_clip_code(ns, d.translation_error, d.rotation_error);
	if (info->status) return true;
	AcRange ranges[LMX_MAX_BONES][7];
	AcBone bones[LMX_MAX_BONES];
	uint32_t code = 0;
	for (uint32_t b = 0; b < nb; ++b) {
		if (d.has_keys && !d.has_keys[b]) continue;
		AcRange* r = ranges[b];
		for (int c = 0; c < 7; ++c) r[c] = ac_range_identity();
		for (uint32_t s = 0; s < ns; ++s) {
			const float* k = keys + ((size_t)s * nb + b) * 7;
			for (int c = 0; c < 3; ++c) ac_range_add_pos(r[c], k[c], d.bind_positions[3 * b + c]);
			for (int c = 3; c < 7; ++c) ac_range_add(r[c], k[c]);
		}
		bones[b] = ac_bone_layout(r, d.bind_positions + 3 * b, d.translation_error, d.rotation_error);
		if (bones[b].code) ac_refuse(code, bones[b].code);
	}
	uint32_t n_ct = 0, n_tt = 0, n_cr = 0, n_rt = 0, t_bits = 0, r_bits = 0;
	for (uint32_t b = 0; b < nb && !code; ++b) {
		if (d.has_keys && !d.has_keys[b]) continue;
		n_ct += bones[b].t_kind == AC_CONST, n_tt += bones[b].t_kind == AC_ANIMATED, t_bits += bones[b].t_entry;
		n_cr += bones[b].r_kind == AC_CONST, n_rt += bones[b].r_kind == AC_ANIMATED, r_bits += bones[b].r_entry;
	}
	if (!code && (t_bits > AC_MAX_FRAME_BITS || r_bits > AC_MAX_FRAME_BITS)) code = LMX_ANIMCOMP_FRAME_BITS;
	if (code) {
		info->status = code;
		return true;
	}
	info->n_const_translations = n_ct, info->n_translations = n_tt, info->n_const_rotations = n_cr, info->n_rotations = n_rt;
	info->translations_frame_size_bits = t_bits, info->rotations_frame_size_bits = r_bits;
	info->translation_stream_size = ((uint64_t)t_bits * ns + 7) / 8;
	info->rotation_stream_size = ((uint64_t)r_bits * ns + 7) / 8;
	if (!out) return true;
	const uint32_t most = n_ct > n_tt ? n_ct : n_tt, most_r = n_cr > n_rt ? n_cr : n_rt;
	if (out->cap_tracks < most || out->cap_tracks < most_r || out->cap_translation_stream < info->translation_stream_size || out->cap_rotation_stream < info->rotation_stream_size) return false;
	if ((n_ct && !out->const_translations) || (n_tt && (!out->translations || !out->translation_stream)) || (n_cr && !out->const_rotations) || (n_rt && (!out->rotations || !out->rotation_stream))) return false;
	if (n_tt) memset(out->translation_stream, 0, (size_t)info->translation_stream_size);
	if (n_rt) memset(out->rotation_stream, 0, (size_t)info->rotation_stream_size);
	// an entry of up to 57 bits at any bit offset: byte by byte, nothing is written behind the stream
	auto put = [](uint8_t* stream, uint64_t at, uint64_t v) {
		uint64_t byte = at >> 3;
		const uint32_t sh = (uint32_t)(at & 7);
		stream[byte++] |= (uint8_t)(v << sh);
		for (v >>= 8 - sh; v; v >>= 8) stream[byte++] |= (uint8_t)v;
	};
	n_ct = n_tt = n_cr = n_rt = t_bits = r_bits = 0;
	for (uint32_t b = 0; b < nb; ++b) {
		if (d.has_keys && !d.has_keys[b]) continue;
		const AcBone& L = bones[b];
		const float* first = keys + (size_t)b * 7;
		AcTrack track;
		if (L.t_kind == AC_CONST) {
			LmxAnimConstTranslation& rec = out->const_translations[n_ct++];
			memset(&rec, 0, sizeof(rec));
			for (int c = 0; c < 3; ++c) rec.value[c] = first[c];
			rec.bone_index = (uint16_t)b;
		} else if (L.t_kind == AC_ANIMATED) {
			ac_translation_records(ranges[b], L, b, t_bits, &out->translations[n_tt++], &track);
			for (uint32_t s = 0; s < ns; ++s) put(out->translation_stream, (uint64_t)info->translations_frame_size_bits * s + t_bits, ac_pack_translation(keys + ((size_t)s * nb + b) * 7, track));
			t_bits += L.t_entry;
		}
		if (L.r_kind == AC_CONST) {
			LmxAnimConstRotation& rec = out->const_rotations[n_cr++];
			memset(&rec, 0, sizeof(rec));
			for (int c = 0; c < 4; ++c) rec.value[c] = first[3 + c];
			rec.bone_index = (uint16_t)b;
		} else if (L.r_kind == AC_ANIMATED) {
			ac_rotation_records(ranges[b], L, b, r_bits, &out->rotations[n_rt++], &track);
			for (uint32_t s = 0; s < ns; ++s) put(out->rotation_stream, (uint64_t)info->rotations_frame_size_bits * s + r_bits, ac_pack_rotation(keys + ((size_t)s * nb + b) * 7 + 3, track));
			r_bits += L.r_entry;
		}
	}
	return true;
}

#if defined(__HIPCC__)
// ---- the device batch (animcomp_kernels.hip) ------------------------------------------------------------------------------------------------
constexpr uint32_t AC_BLOCK = 256;
constexpr uint32_t AC_RANGE_SAMPLES = 64;                                   // of one workgroup of the range fold
constexpr uint32_t AC_GROUP_FRAMES = 32;                                    // 32 frames of any size are a whole number of dwords
constexpr uint32_t AC_GROUP_WORDS = LMX_MAX_BONES * AC_MAX_ENTRY_BITS;      // ... frame_size_bits of them: at most 11172 (44688 bytes of LDS)
constexpr uint32_t AC_PACK_ENTRIES = 8192;                                  // a pack workgroup takes groups up to about this many entries

struct AcClip {
	uint32_t n_bones, n_samples;
	uint32_t bone_off;  // the bones of the clips before it: where its per-bone inputs and its track records start
	uint32_t part_off;  // of its partial folds: n_chunks x n_bones x 7
	uint64_t key_off;   // in records
	float t_error, r_error;
};
struct AcRangeItem { // one workgroup of the range fold: samples chunk * AC_RANGE_SAMPLES .. of a clip
	uint32_t clip, chunk;
};
struct AcPackItem { // one workgroup of the pack: groups group0 .. group0 + n_groups - 1 of one stream of a clip
	uint32_t clip, rotation, group0, n_groups;
	uint32_t out_word, _pad; // where the clip's stream starts, in dwords
};
struct AcBatch {
	const AcClip* clips;
	const float* keys;       // 7 floats per record
	const uint8_t* has_keys; // per bone of the batch
	const float* bind;       // 3 floats per bone of the batch
	AcRange* partials;
	LmxAnimCompInfo* infos;
	LmxAnimConstTranslation* ct;
	LmxAnimTranslationTrack* tt;
	LmxAnimConstRotation* cr;
	LmxAnimRotationTrack* rt;
	AcTrack* t_tracks;
	AcTrack* r_tracks;
};

hipError_t launch_animcomp_ranges(hipStream_t s, const AcBatch& batch, const AcRangeItem* items, uint32_t n_items);
hipError_t launch_animcomp_layout(hipStream_t s, const AcBatch& batch, uint32_t n_clips);
hipError_t launch_animcomp_pack(hipStream_t s, const AcBatch& batch, const AcPackItem* items, uint32_t n_items, uint32_t* t_stream, uint32_t* r_stream);
#endif

} // namespace lmx
