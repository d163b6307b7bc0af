// lmx_capi_anim.hip — animation sampling entry points (include/lumix_mi355.h, "animation" section): Animation resources are
// flattened into concatenated device tables, every skinned instance is an Animable {animation, time}, and lmx_anim_update is
// AnimationModuleImpl::updateAnimable for all of them at once; its output is the relative pose lmx_skin_run consumes.
#include <cmath>

#include "lmx_context.h"

using namespace lmx;

namespace lmx {

int anim_upload_tables(LmxContext* ctx) {
	AnimState& an = ctx->anim;
	if (!an.tables_dirty) return LMX_OK;
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking(an.d_anims, an.anims));
	LMX_HIP(ctx, upload_blocking(an.d_src, an.src));
	LMX_HIP(ctx, upload_blocking(an.d_ct, an.ct));
	LMX_HIP(ctx, upload_blocking(an.d_tt, an.tt));
	LMX_HIP(ctx, upload_blocking(an.d_cr, an.cr));
	LMX_HIP(ctx, upload_blocking(an.d_rt, an.rt));
	LMX_HIP(ctx, upload_blocking(an.d_tstream, an.tstream));
	LMX_HIP(ctx, upload_blocking(an.d_rstream, an.rstream));
	for (const AnimDeviceStream& d : an.device_streams) LMX_HIP(ctx, device_copy_blocking((d.rotation ? an.d_rstream.p : an.d_tstream.p) + d.at, (const uint8_t*)d.copy.p, d.bytes));
	LMX_HIP(ctx, upload_blocking(an.d_root_t, an.root_t));
	LMX_HIP(ctx, upload_blocking(an.d_root_r, an.root_r));
	LMX_HIP(ctx, upload_blocking(an.d_rel_pos, an.rel_pos));
	LMX_HIP(ctx, upload_blocking(an.d_rel_rot, an.rel_rot));
	an.tables_dirty = false;
	return LMX_OK;
}

} // namespace lmx

namespace {

// lmx_anim_add; d_streams: the clip's two streams are on the device (translation, rotation; a->translation_stream / rotation_stream are not read)
int anim_add(LmxContext* ctx, const LmxAnimation* a, uint32_t* out_animation, const uint8_t* const* d_streams) {
	if (!a || !out_animation) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null animation / out");
	if (!(a->fps > 0.f) || !a->frame_count || !a->length) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "fps, frame_count and length must be positive");
	if ((a->n_const_translations && !a->const_translations) || (a->n_translations && !a->translations) || (a->n_const_rotations && !a->const_rotations) ||
		(a->n_rotations && !a->rotations))
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null track array");
	// all stream arithmetic in 64 bits. The caller holds frame_count + 1 frames (animation.cpp:464); the tables store frame_count + 2 (below), and
	// the kernel addresses a frame's bits with a 32-bit offset and reads 64 bits from it
	const uint64_t frames_in = (uint64_t)a->frame_count + 1, frames_stored = (uint64_t)a->frame_count + 2;
	const uint64_t t_bits = (uint64_t)a->translations_frame_size_bits * frames_in, r_bits = (uint64_t)a->rotations_frame_size_bits * frames_in;
	if ((uint64_t)a->translations_frame_size_bits * frames_stored + 64 > 0xFFFFFFFFull || (uint64_t)a->rotations_frame_size_bits * frames_stored + 64 > 0xFFFFFFFFull)
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frame size %u / %u bits x (frame_count %u + 2) frames does not fit a 32-bit bit offset", a->translations_frame_size_bits,
			a->rotations_frame_size_bits, a->frame_count);
	// The sample point's upper clamp is (float)frame_count - 0.00001f (anim_kernels.hip, animation.cpp:132). Up to 2^24 every count is an fp32 number
	// and the clamp is at most frame_count; above, (float)frame_count can round up and sample_idx would pass the frames stored here
	if (a->frame_count > (1u << 24)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "frame_count %u exceeds 2^24: the sample point is computed in fp32", a->frame_count);
	const uint64_t t_need = (t_bits + 7) / 8, r_need = (r_bits + 7) / 8;
	const uint8_t* t_src = d_streams ? d_streams[0] : a->translation_stream;
	const uint8_t* r_src = d_streams ? d_streams[1] : a->rotation_stream;
	if ((a->n_translations && (!t_src || a->translation_stream_size < t_need)) || (a->n_rotations && (!r_src || a->rotation_stream_size < r_need)))
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "track streams must hold frame_count + 1 frames (animation.cpp:464): need %llu / %llu bytes", (unsigned long long)t_need, (unsigned long long)r_need);
	if ((a->root_translation_track >= 0 && ((uint32_t)a->root_translation_track >= a->n_translations || !a->root_pose_translations)) ||
		(a->root_rotation_track >= 0 && ((uint32_t)a->root_rotation_track >= a->n_rotations || !a->root_pose_rotations)))
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "root-motion track index out of range or pose arrays missing");
	AnimState& an = ctx->anim;
	uint32_t max_bone = 0; // m_max_accessed_bone_index, animation.cpp:369-393
	for (uint32_t i = 0; i < a->n_const_translations; ++i) max_bone = std::max<uint32_t>(max_bone, a->const_translations[i].bone_index);
	for (uint32_t i = 0; i < a->n_translations; ++i) max_bone = std::max<uint32_t>(max_bone, a->translations[i].bone_index);
	for (uint32_t i = 0; i < a->n_const_rotations; ++i) max_bone = std::max<uint32_t>(max_bone, a->const_rotations[i].bone_index);
	for (uint32_t i = 0; i < a->n_rotations; ++i) max_bone = std::max<uint32_t>(max_bone, a->rotations[i].bone_index);
	if (max_bone >= LMX_MAX_BONES) return fail(ctx, LMX_ERR_CAPACITY, "track bone index %u >= %d (Model::Bone::MAX_COUNT)", max_bone, LMX_MAX_BONES);
	const uint64_t t_store = a->n_translations ? ((uint64_t)a->translations_frame_size_bits * frames_stored + 7) / 8 : 0;
	const uint64_t r_store = a->n_rotations ? ((uint64_t)a->rotations_frame_size_bits * frames_stored + 7) / 8 : 0;
	if (an.tstream.size() + t_store + 24 > 0xFFFFFFFFull || an.rstream.size() + r_store + 24 > 0xFFFFFFFFull || an.root_r.size() + frames_stored > 0xFFFFFFFFull)
		return fail(ctx, LMX_ERR_CAPACITY, "the animation tables are addressed with 32-bit offsets: no room for this clip");
	// per-bone sources: the reference runs the four track lists in order; with at most one translation and one rotation source per
	// bone the order is irrelevant and a lane can look its bone up directly
	std::vector<int32_t> src(2 * (size_t)(max_bone + 1), -1);
	auto claim = [&](uint32_t bone, int which, int32_t code) {
		int32_t& s = src[2 * bone + which];
		if (s != -1) return false;
		s = code;
		return true;
	};
	for (uint32_t i = 0; i < a->n_const_translations; ++i)
		if (!claim(a->const_translations[i].bone_index, 0, (int32_t)(2 * i))) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bone %u has two translation tracks", a->const_translations[i].bone_index);
	for (uint32_t i = 0; i < a->n_translations; ++i) {
		const LmxAnimTranslationTrack& t = a->translations[i];
		if (!claim(t.bone_index, 0, (int32_t)(2 * i + 1))) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bone %u has two translation tracks", t.bone_index);
		if (t.bitsizes[0] + t.bitsizes[1] + t.bitsizes[2] > 57u) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "translation track %u: more than 57 bits per frame cannot be read with one 64-bit load (animation.cpp:323-325)", i);
		if (t.offset_bits + t.bitsizes[0] + t.bitsizes[1] + t.bitsizes[2] > a->translations_frame_size_bits) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "translation track %u exceeds the frame size", i);
	}
	for (uint32_t i = 0; i < a->n_const_rotations; ++i)
		if (!claim(a->const_rotations[i].bone_index, 1, (int32_t)(2 * i))) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bone %u has two rotation tracks", a->const_rotations[i].bone_index);
	for (uint32_t i = 0; i < a->n_rotations; ++i) {
		const LmxAnimRotationTrack& t = a->rotations[i];
		if (!claim(t.bone_index, 1, (int32_t)(2 * i + 1))) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bone %u has two rotation tracks", t.bone_index);
		if (1u + t.bitsizes[0] + t.bitsizes[1] + t.bitsizes[2] > 57u) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "rotation track %u: more than 57 bits per frame", i);
		if (t.offset_bits + 1u + t.bitsizes[0] + t.bitsizes[1] + t.bitsizes[2] > a->rotations_frame_size_bits) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "rotation track %u exceeds the frame size", i);
		if (t.skipped_channel > 3) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "rotation track %u: skipped_channel %u", i, t.skipped_channel);
	}
	// a device stream gets the library's own copy first: nothing below can fail once the tables have grown
	AnimDeviceStream own[2];
	if (d_streams) {
		const uint64_t need[2] = {t_store ? t_need : 0, r_store ? r_need : 0};
		for (int k = 0; k < 2; ++k) {
			own[k].rotation = k == 1;
			own[k].bytes = (size_t)need[k];
			if (!need[k]) continue;
			LMX_HIP(ctx, own[k].copy.reserve((size_t)need[k]));
			LMX_HIP(ctx, device_copy_on_stream(own[k].copy.p, d_streams[k], (size_t)need[k], ctx->stream));
		}
	}
	AnimDevice d;
	memset(&d, 0, sizeof(d));
	d.fps = a->fps; d.frame_count = a->frame_count; d.length = a->length; d.tfs_bits = a->translations_frame_size_bits; d.rfs_bits = a->rotations_frame_size_bits;
	d.max_bone = max_bone;
	d.src_off = (uint32_t)an.src.size();
	d.ct_off = (uint32_t)an.ct.size(); d.tt_off = (uint32_t)an.tt.size(); d.cr_off = (uint32_t)an.cr.size(); d.rt_off = (uint32_t)an.rt.size();
	d.tstream_off = (uint32_t)an.tstream.size(); d.rstream_off = (uint32_t)an.rstream.size();
	d.root_translation_track = a->root_translation_track; d.root_rotation_track = a->root_rotation_track;
	d.root_off = (uint32_t)(an.root_r.size());
	an.src.insert(an.src.end(), src.begin(), src.end());
	an.ct.insert(an.ct.end(), a->const_translations, a->const_translations + a->n_const_translations);
	an.tt.insert(an.tt.end(), a->translations, a->translations + a->n_translations);
	an.cr.insert(an.cr.end(), a->const_rotations, a->const_rotations + a->n_const_rotations);
	an.rt.insert(an.rt.end(), a->rotations, a->rotations + a->n_rotations);
	// The frame after the last reads as zero bits: a sample at the clip's end (sample_idx == frame_count, f == 0, every frame_count >= 257: the
	// sample point's upper clamp frame_count - 0.00001f is frame_count in fp32) decodes frames frame_count and frame_count + 1, which the
	// reference leaves to whatever follows its stream. So: the caller's frame_count + 1 frames to the bit (the tail of their last byte is
	// cleared), one more frame of zero bits, then 16 bytes of slack for the 64-bit reads; every clip starts 8-byte aligned.
	// (a device stream: zeros stand in its place here, and the copy above is laid over them whenever the tables go up; the compressor has
	// cleared the tail of its last byte)
	auto append_stream = [](std::vector<uint8_t>& dst, const uint8_t* src_bytes, uint64_t bits, uint64_t need, uint64_t store) {
		const size_t start = dst.size();
		if (store) {
			if (src_bytes) {
				dst.insert(dst.end(), src_bytes, src_bytes + need);
				if (bits & 7) dst.back() &= (uint8_t)((1u << (bits & 7)) - 1u);
			}
			dst.resize(start + store, 0);
		}
		dst.resize((dst.size() + 16 + 7) & ~(size_t)7, 0);
	};
	append_stream(an.tstream, d_streams ? nullptr : a->translation_stream, t_bits, t_need, t_store);
	append_stream(an.rstream, d_streams ? nullptr : a->rotation_stream, r_bits, r_need, r_store);
	if (d_streams) {
		own[0].at = d.tstream_off, own[1].at = d.rstream_off;
		for (int k = 0; k < 2; ++k)
			if (own[k].bytes) an.device_streams.push_back(std::move(own[k]));
	}
	for (size_t f = 0; f < (size_t)frames_in; ++f) { // frame_count + 1 entries of the caller's, then one of zeros (the same definition)
		for (int k = 0; k < 3; ++k) an.root_t.push_back(a->root_translation_track >= 0 ? a->root_pose_translations[3 * f + k] : 0.f);
		an.root_r.push_back(a->root_rotation_track >= 0 ? make_float4(a->root_pose_rotations[4 * f], a->root_pose_rotations[4 * f + 1], a->root_pose_rotations[4 * f + 2], a->root_pose_rotations[4 * f + 3])
		                                                : make_float4(0.f, 0.f, 0.f, 1.f));
	}
	for (int k = 0; k < 3; ++k) an.root_t.push_back(0.f);
	an.root_r.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
	*out_animation = (uint32_t)an.anims.size();
	an.anims.push_back(d);
	an.tables_dirty = true;
	return LMX_OK;
}

} // namespace

extern "C" {

int lmx_anim_add(LmxContext* ctx, const LmxAnimation* a, uint32_t* out_animation) {
	LMX_CHECK_CTX(ctx);
	return anim_add(ctx, a, out_animation, nullptr);
}

int lmx_anim_add_compressed(LmxContext* ctx, LmxAnimCompressor* ac, uint32_t clip, uint32_t length, uint32_t* out_animation) {
	LMX_CHECK_CTX(ctx);
	if (!ac || !out_animation) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null compressor / out");
	AnimCompClipView v;
	if (int rc = animcomp_clip_view(ctx, ac, clip, &v)) return rc;
	LmxAnimation a;
	memset(&a, 0, sizeof(a));
	a.fps = v.fps, a.frame_count = v.info.frame_count, a.length = length;
	a.translations_frame_size_bits = v.info.translations_frame_size_bits, a.rotations_frame_size_bits = v.info.rotations_frame_size_bits;
	a.n_const_translations = v.info.n_const_translations, a.n_translations = v.info.n_translations, a.n_const_rotations = v.info.n_const_rotations, a.n_rotations = v.info.n_rotations;
	a.const_translations = v.ct.data(), a.translations = v.tt.data(), a.const_rotations = v.cr.data(), a.rotations = v.rt.data();
	a.translation_stream_size = v.info.translation_stream_size, a.rotation_stream_size = v.info.rotation_stream_size;
	a.root_translation_track = a.root_rotation_track = -1;
	const uint8_t* d_streams[2] = {v.d_translation_stream, v.d_rotation_stream};
	return anim_add(ctx, &a, out_animation, d_streams);
}

int lmx_anim_set_model_pose(LmxContext* ctx, uint32_t model, const LmxLocalRigidTransform* relative, uint32_t n_bones) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	if (model >= sk.models.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown skin model %u", model);
	if (!relative || n_bones != sk.models[model].n_bones) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "model %u has %u bones", model, sk.models[model].n_bones);
	const size_t total = sk.parents.size(); // bones of all models
	an.rel_pos.resize(total * 3, 0.f);
	an.rel_rot.resize(total, make_float4(0.f, 0.f, 0.f, 1.f));
	const uint32_t off = sk.models[model].bone_offset;
	for (uint32_t b = 0; b < n_bones; ++b) {
		for (int k = 0; k < 3; ++k) an.rel_pos[3 * (size_t)(off + b) + k] = relative[b].pos[k];
		an.rel_rot[off + b] = make_float4(relative[b].rot[0], relative[b].rot[1], relative[b].rot[2], relative[b].rot[3]);
	}
	an.tables_dirty = true;
	return LMX_OK;
}

int lmx_anim_set_animables(LmxContext* ctx, uint32_t n_instances, const uint32_t* animation, const uint32_t* time) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	if (n_instances != sk.inst.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the skin instance table has %zu instances", sk.inst.size());
	if (n_instances && (!animation || !time)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null animation / time array");
	for (uint32_t i = 0; i < n_instances; ++i)
		if (animation[i] != LMX_ANIM_NONE && animation[i] >= an.anims.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: unknown animation %u", i, animation[i]);
	LMX_HIP(ctx, an.d_anim_of.reserve(std::max<size_t>(n_instances, 1)));
	LMX_HIP(ctx, an.d_time_of.reserve(std::max<size_t>(n_instances, 1)));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking(an.d_anim_of.p, animation, n_instances));
	LMX_HIP(ctx, upload_blocking(an.d_time_of.p, time, n_instances));
	an.n_animables = n_instances;
	return LMX_OK;
}

int lmx_anim_set_weight(LmxContext* ctx, float weight) {
	LMX_CHECK_CTX(ctx);
	if (!(weight >= 0.f && weight <= 1.f)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "weight %g outside [0, 1]", (double)weight);
	ctx->anim.weight = weight;
	return LMX_OK;
}

int lmx_anim_update(LmxContext* ctx, float time_delta) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	// Time::fromSeconds is u32(seconds * ONE_SECOND): out of range the conversion is undefined and differs between the host and the device
	if (!std::isfinite(time_delta) || !(std::fabs(time_delta) * (float)LMX_TIME_ONE_SECOND < 4294967296.f))
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "time_delta %g: not finite, or more than 2^32 ticks of 1 / %u s", (double)time_delta, LMX_TIME_ONE_SECOND);
	if (sk.inst.empty()) return LMX_OK;
	if (an.n_animables != sk.inst.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_anim_set_animables has not been called for this instance table");
	if (an.rel_rot.size() != sk.parents.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_anim_set_model_pose is missing for a model added later");
	if (int rc = anim_upload_tables(ctx)) return rc;
	AnimTables t;
	t.src = an.d_src.p; t.const_translations = an.d_ct.p; t.translations = an.d_tt.p; t.const_rotations = an.d_cr.p; t.rotations = an.d_rt.p;
	t.translation_stream = an.d_tstream.p; t.rotation_stream = an.d_rstream.p; t.root_translations = an.d_root_t.p; t.root_rotations = an.d_root_r.p;
	ProfScope ps(ctx, LMX_K_ANIM_UPDATE);
	LMX_HIP(ctx, launch_anim_update(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, an.d_anim_of.p, an.d_time_of.p, time_delta, an.weight,
		an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	// the library's pose buffers hold fresh relative poses: the source of the next lmx_skin_run
	sk.borrowed_pos = nullptr;
	sk.borrowed_rot = nullptr;
	sk.poses_uploaded = true;
	sk.pose_is_absolute = false;
	return LMX_OK;
}

int lmx_anim_eval_blend_stacks(LmxContext* ctx, uint32_t n_instances, const uint32_t* first_sample, const LmxBlendSample* samples) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	if (n_instances != sk.inst.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the skin instance table has %zu instances", sk.inst.size());
	if (!n_instances) return LMX_OK;
	if (!first_sample) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null first_sample");
	if (an.rel_rot.size() != sk.parents.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_anim_set_model_pose is missing for a model added later");
	for (uint32_t i = 0; i < n_instances; ++i)
		if (first_sample[i + 1] < first_sample[i]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "first_sample decreases at instance %u", i);
	const uint32_t n_samples = first_sample[n_instances];
	if (first_sample[0] != 0 || (n_samples && !samples)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "first_sample[0] must be 0 and samples non-null");
	for (uint32_t k = 0; k < n_samples; ++k) {
		if (samples[k].animation >= an.anims.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "sample %u: unknown animation %u", k, samples[k].animation);
		if (!(samples[k].weight >= 0.f && samples[k].weight <= 1.f)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "sample %u: weight %g outside [0, 1]", k, (double)samples[k].weight);
	}
	if (int rc = anim_upload_tables(ctx)) return rc;
	LMX_HIP(ctx, an.d_first_sample.reserve((size_t)n_instances + 1));
	LMX_HIP(ctx, an.d_samples.reserve(std::max<size_t>(n_samples, 1)));
	// the caller's arrays are pageable: the copies below complete before this returns, and the stream orders them against the
	// previous frame's kernel that still reads the same device buffers
	LMX_HIP(ctx, upload_on_stream(an.d_first_sample.p, first_sample, (size_t)n_instances + 1, ctx->stream));
	LMX_HIP(ctx, upload_on_stream(an.d_samples.p, samples, n_samples, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	AnimTables t;
	t.src = an.d_src.p; t.const_translations = an.d_ct.p; t.translations = an.d_tt.p; t.const_rotations = an.d_cr.p; t.rotations = an.d_rt.p;
	t.translation_stream = an.d_tstream.p; t.rotation_stream = an.d_rstream.p; t.root_translations = an.d_root_t.p; t.root_rotations = an.d_root_r.p;
	ProfScope ps(ctx, LMX_K_ANIM_UPDATE);
	LMX_HIP(ctx, launch_anim_blend_stack(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, (uint32_t)an.anims.size(), an.d_samples.p,
		an.d_first_sample.p, an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	sk.borrowed_pos = nullptr;
	sk.borrowed_rot = nullptr;
	sk.poses_uploaded = true;
	sk.pose_is_absolute = false;
	return LMX_OK;
}

int lmx_anim_eval_blend_instrs(LmxContext* ctx, uint32_t n_instances, const uint32_t* first_instr, const LmxBlendInstr* instrs) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	if (n_instances != sk.inst.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the skin instance table has %zu instances", sk.inst.size());
	if (!n_instances) return LMX_OK;
	if (!first_instr) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null first_instr");
	if (an.rel_rot.size() != sk.parents.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_anim_set_model_pose is missing for a model added later");
	for (uint32_t i = 0; i < n_instances; ++i)
		if (first_instr[i + 1] < first_instr[i]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "first_instr decreases at instance %u", i);
	const uint32_t n_instrs = first_instr[n_instances];
	if (first_instr[0] != 0 || (n_instrs && !instrs)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "first_instr[0] must be 0 and instrs non-null");
	// the kernel carries no checks of its own: everything it indexes with is validated here
	// (one pass over the records: a call without IK runs k_anim_blend_stack on the SAMPLE fields, gathered here into their 16-byte form)
	bool any_ik = false;
	an.samples_scratch.resize(n_instrs);
	for (uint32_t i = 0; i < n_instances; ++i) {
		for (uint32_t k = first_instr[i]; k < first_instr[i + 1]; ++k) {
			const LmxBlendInstr& ins = instrs[k];
			if (ins.op == LMX_BLEND_SAMPLE) {
				if (ins.animation >= an.anims.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: unknown animation %u", k, ins.animation);
				if (!(ins.weight >= 0.f && ins.weight <= 1.f)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: weight %g outside [0, 1]", k, (double)ins.weight);
				if (!any_ik) an.samples_scratch[k] = LmxBlendSample{ins.animation, ins.weight, ins.time, ins.looped};
			} else if (ins.op == LMX_BLEND_IK) {
				const SkinInstance& in = sk.inst[i];
				any_ik = true;
				if (!std::isfinite(ins.alpha) || !std::isfinite(ins.target[0]) || !std::isfinite(ins.target[1]) || !std::isfinite(ins.target[2]))
					return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: non-finite IK alpha or target", k);
				if (!ins.bones_count || ins.bones_count > LMX_IK_MAX_BONES)
					return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: IK bones_count %u not in [1, %d] (MAX_BONES_COUNT, controller.cpp:171)", k, ins.bones_count, LMX_IK_MAX_BONES);
				if (ins.leaf_bone == LMX_BONE_NONE) continue; // leaf not found: the instruction does nothing (controller.cpp:180-183)
				if (ins.leaf_bone >= in.n_bones) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: IK leaf bone %u, the model of instance %u has %u bones", k, ins.leaf_bone, i, in.n_bones);
				int32_t b = (int32_t)ins.leaf_bone;
				for (uint32_t up = 1; up < ins.bones_count; ++up) {
					b = sk.parents[in.model_offset + (uint32_t)b];
					if (b < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: IK chain of %u bones walks past the root (bone %u has %u ancestors)", k, ins.bones_count, ins.leaf_bone, up - 1);
				}
			} else return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instruction %u: unknown op %u", k, ins.op);
		}
	}
	if (int rc = anim_upload_tables(ctx)) return rc;
	AnimTables t;
	t.src = an.d_src.p; t.const_translations = an.d_ct.p; t.translations = an.d_tt.p; t.const_rotations = an.d_cr.p; t.rotations = an.d_rt.p;
	t.translation_stream = an.d_tstream.p; t.rotation_stream = an.d_rstream.p; t.root_translations = an.d_root_t.p; t.root_rotations = an.d_root_r.p;
	LMX_HIP(ctx, an.d_first_sample.reserve((size_t)n_instances + 1));
	if (!any_ik) { // SAMPLE records only: k_anim_blend_stack on their 16-byte form
		LMX_HIP(ctx, an.d_samples.reserve(std::max<size_t>(n_instrs, 1)));
		LMX_HIP(ctx, upload_on_stream(an.d_first_sample.p, first_instr, (size_t)n_instances + 1, ctx->stream));
		LMX_HIP(ctx, upload_on_stream(an.d_samples.p, an.samples_scratch.data(), n_instrs, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		ProfScope ps(ctx, LMX_K_ANIM_UPDATE);
		LMX_HIP(ctx, launch_anim_blend_stack(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, (uint32_t)an.anims.size(), an.d_samples.p,
			an.d_first_sample.p, an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	} else {
		LMX_HIP(ctx, an.d_instrs.reserve(std::max<size_t>(n_instrs, 1)));
		if (an.parents_uploaded != sk.parents.size()) { // models only append; the previous frame's kernel may still read the old copy
			LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
			LMX_HIP(ctx, upload_blocking(an.d_parents, sk.parents.data(), sk.parents.size()));
			an.parents_uploaded = sk.parents.size();
		}
		// pageable host arrays: the copies complete before this returns, ordered by the stream against the previous frame's kernel
		LMX_HIP(ctx, upload_on_stream(an.d_first_sample.p, first_instr, (size_t)n_instances + 1, ctx->stream));
		LMX_HIP(ctx, upload_on_stream(an.d_instrs.p, instrs, n_instrs, ctx->stream));
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		ProfScope ps(ctx, LMX_K_ANIM_UPDATE);
		LMX_HIP(ctx, launch_anim_blend_instrs(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, (uint32_t)an.anims.size(), an.d_instrs.p,
			an.d_first_sample.p, an.d_parents.p, an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	}
	sk.borrowed_pos = nullptr;
	sk.borrowed_rot = nullptr;
	sk.poses_uploaded = true;
	sk.pose_is_absolute = false;
	return LMX_OK;
}

int lmx_anim_read_times(LmxContext* ctx, uint32_t* time, uint32_t n_instances) {
	LMX_CHECK_CTX(ctx);
	AnimState& an = ctx->anim;
	if (n_instances != an.n_animables || (n_instances && !time)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "expected %u animables", an.n_animables);
	return read_now(ctx, time, (const uint32_t*)an.d_time_of.p, n_instances);
}

int lmx_anim_read_pose(LmxContext* ctx, uint32_t instance, float* out_pos, float* out_rot, uint32_t cap_bones) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	if (instance >= sk.inst.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad instance");
	const SkinInstance& in = sk.inst[instance];
	if (cap_bones < in.n_bones) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u bones", in.n_bones);
	if (sk.pose_is_absolute || !sk.poses_uploaded || sk.borrowed_pos) return fail(ctx, LMX_ERR_NOT_BUILT, "the pose buffers do not hold a relative pose (call after lmx_anim_update, before lmx_skin_run)");
	LMX_HIP(ctx, read_back(out_pos, sk.d_pose_pos.p + (size_t)in.bone_offset * 3, (size_t)in.n_bones * 3, ctx->stream));
	return read_now(ctx, (float4*)out_rot, (const float4*)sk.d_pose_rot.p + in.bone_offset, in.n_bones);
}

} // extern "C"
