// lmx_capi_animators.hip — Animator entry points (include/lumix_mi355.h, "animator controllers" section): compiled controller resources
// become device-resident programs (lmx_controller_program.cpp), every skin instance may carry an Animator, and lmx_animators_update is the
// first half of AnimationModuleImpl::updateAnimator for all of them: Controller::update on the device, its instructions packed on the
// device and handed to k_anim_blend_instrs, root motion left in device memory for lmx_animators_apply_root_motion.
#include <cmath>

#include <hipcub/hipcub.hpp>

#include "lmx_context.h"

using namespace lmx;

namespace {

uint64_t pair_key(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | b; }

int upload_clips(LmxContext* ctx) {
	AnimState& an = ctx->anim;
	AnimatorsState& as = ctx->animators;
	if (!as.clips_dirty && as.clips_uploaded == an.anims.size()) return LMX_OK;
	std::vector<CtlClip> clips(an.anims.size());
	for (size_t i = 0; i < clips.size(); ++i) {
		clips[i].fps = an.anims[i].fps;
		clips[i].frame_count = an.anims[i].frame_count;
		clips[i].length = an.anims[i].length;
		clips[i].rm_t = i < as.rm_t_of.size() ? as.rm_t_of[i] : LMX_ANIM_NONE;
		clips[i].rm_r = i < as.rm_r_of.size() ? as.rm_r_of[i] : LMX_ANIM_NONE;
	}
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking(as.d_clips, clips));
	LMX_HIP(ctx, upload_blocking(as.d_rm_t, as.rm_t));
	LMX_HIP(ctx, upload_blocking(as.d_rm_r, as.rm_r));
	as.clips_dirty = false;
	as.clips_uploaded = clips.size();
	return LMX_OK;
}

// the place of Animator `a`'s inputs and their count
void input_range(const AnimatorsState& as, uint32_t first, uint32_t n, uint32_t& base, uint32_t& count) {
	base = first < as.n ? as.animators[first].input_base : as.total_inputs;
	const uint32_t end = first + n < as.n ? as.animators[first + n].input_base : as.total_inputs;
	count = end - base;
}

} // namespace

extern "C" {

int lmx_anim_controller_add(LmxContext* ctx, const void* bytes, uint64_t n_bytes, uint32_t* out_controller) {
	LMX_CHECK_CTX(ctx);
	if (!bytes || !out_controller) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null bytes / out");
	ControllerHost c;
	std::string error;
	if (!controller_program_parse((const uint8_t*)bytes, n_bytes, c.prog, error)) return fail(ctx, LMX_ERR_INVALID, "controller: %s", error.c_str());
	*out_controller = (uint32_t)ctx->animators.controllers.size();
	ctx->animators.controllers.push_back(std::move(c));
	return LMX_OK;
}

int lmx_anim_controller_input_types(LmxContext* ctx, uint32_t controller, uint32_t* out_types, uint32_t capacity, uint32_t* out_count) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (controller >= as.controllers.size() || !out_count) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown controller %u / null out_count", controller);
	const std::vector<uint32_t>& types = as.controllers[controller].prog.input_types;
	*out_count = (uint32_t)types.size();
	if (!out_types) return LMX_OK;
	if (capacity < types.size()) return fail(ctx, LMX_ERR_CAPACITY, "need room for %zu types", types.size());
	if (!types.empty()) memcpy(out_types, types.data(), 4 * types.size());
	return LMX_OK;
}

int lmx_anim_controller_set_slots(LmxContext* ctx, uint32_t controller, uint32_t set, const uint32_t* slot_animation, uint32_t n_slots) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (controller >= as.controllers.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown controller %u", controller);
	ControllerHost& c = as.controllers[controller];
	if (n_slots != c.prog.n_slots || (n_slots && !slot_animation)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "controller %u has %u animation slots", controller, c.prog.n_slots);
	for (uint32_t i = 0; i < n_slots; ++i) {
		if (slot_animation[i] == LMX_ANIM_NONE) {
			// the reference dereferences the null Animation* there (nodes.cpp:678, getPose's ASSERT(anim), controller.cpp:144)
			if (c.prog.slot_required[i]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "slot %u is named by an ANIMATION or BLEND1D node and cannot be empty", i);
		} else if (slot_animation[i] >= ctx->anim.anims.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "slot %u: unknown animation %u", i, slot_animation[i]);
	}
	c.sets[set].assign(slot_animation, slot_animation + n_slots);
	auto at = as.slots_at.find(pair_key(controller, set));
	if (as.is_set && at != as.slots_at.end()) { // Animators run on this table: the previous frame's kernel may still read it
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		LMX_HIP(ctx, upload_blocking(as.d_slots.p + at->second, slot_animation, n_slots));
	}
	return LMX_OK;
}

int lmx_anim_set_root_motion(LmxContext* ctx, uint32_t animation, const float* translations, const float* rotations) {
	LMX_CHECK_CTX(ctx);
	AnimState& an = ctx->anim;
	AnimatorsState& as = ctx->animators;
	if (animation >= an.anims.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "unknown animation %u", animation);
	const size_t entries = (size_t)an.anims[animation].frame_count + 1;
	if (as.rm_t.size() / 3 + entries > 0x7fffffffull || as.rm_r.size() / 4 + entries > 0x7fffffffull) return fail(ctx, LMX_ERR_CAPACITY, "the root-motion tables are addressed with 32-bit offsets");
	as.rm_t_of.resize(an.anims.size(), LMX_ANIM_NONE);
	as.rm_r_of.resize(an.anims.size(), LMX_ANIM_NONE);
	as.rm_t_of[animation] = as.rm_r_of[animation] = LMX_ANIM_NONE; // (a clip set again appends: tables only grow)
	if (translations) {
		as.rm_t_of[animation] = (uint32_t)(as.rm_t.size() / 3);
		as.rm_t.insert(as.rm_t.end(), translations, translations + 3 * entries);
	}
	if (rotations) {
		as.rm_r_of[animation] = (uint32_t)(as.rm_r.size() / 4);
		as.rm_r.insert(as.rm_r.end(), rotations, rotations + 4 * entries);
	}
	as.clips_dirty = true;
	return LMX_OK;
}

int lmx_animators_set(LmxContext* ctx, uint32_t n_instances, const uint32_t* controller, const uint32_t* set, const uint32_t* flags, const int32_t* entity,
	const uint64_t* bone_hashes, uint32_t n_bone_hashes) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimatorsState& as = ctx->animators;
	if (n_instances != sk.inst.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "the skin instance table has %zu instances", sk.inst.size());
	if (n_instances && (!controller || !set || !flags || !entity)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null controller / set / flags / entity array");
	size_t pose_bones = 0; // the bones of every instance, as the pose arrays hold them
	for (const SkinInstance& in : sk.inst) pose_bones = std::max<size_t>(pose_bones, (size_t)in.bone_offset + in.n_bones);
	if (bone_hashes ? n_bone_hashes != pose_bones : n_bone_hashes != 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bone_hashes holds one hash per bone of every instance (%zu), or is null", pose_bones);
	// everything is validated and built on the side; the running state is replaced at the end
	std::vector<CtlAnimator> animators(n_instances);
	std::vector<uint32_t> order, slots, ik_leaf, input_types, rm_animator;
	std::vector<int32_t> rm_entity;
	std::unordered_map<uint64_t, uint32_t> slots_at, ik_at;
	std::vector<uint32_t> per_controller(as.controllers.size(), 0);
	std::unordered_map<int32_t, uint32_t> rm_seen;
	for (uint32_t i = 0; i < n_instances; ++i) {
		CtlAnimator& a = animators[i];
		memset(&a, 0, sizeof(a));
		a.controller = controller[i];
		a.flags = flags[i];
		a.input_base = (uint32_t)input_types.size();
		if (flags[i] & ~LMX_ANIMATOR_USE_ROOT_MOTION) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: unknown flags %#x", i, flags[i]);
		if (controller[i] == LMX_CONTROLLER_NONE) continue;
		if (controller[i] >= as.controllers.size()) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: unknown controller %u", i, controller[i]);
		const ControllerHost& c = as.controllers[controller[i]];
		const SkinInstance& in = sk.inst[i];
		++per_controller[controller[i]];
		const uint64_t sk_key = pair_key(controller[i], set[i]);
		auto s_at = slots_at.find(sk_key);
		if (s_at == slots_at.end()) {
			auto have = c.sets.find(set[i]);
			if (have == c.sets.end()) return fail(ctx, LMX_ERR_NOT_BUILT, "instance %u: lmx_anim_controller_set_slots has not been called for controller %u, set %u", i, controller[i], set[i]);
			s_at = slots_at.emplace(sk_key, (uint32_t)slots.size()).first;
			slots.insert(slots.end(), have->second.begin(), have->second.end());
		}
		a.slots_off = s_at->second;
		// IKNode's per-model work, once per (controller, model): the leaf's bone index (Model::getBoneIndex, controller.cpp:179-183) and the chain rules
		const uint64_t ik_key = pair_key(controller[i], in.model_offset);
		auto i_at = ik_at.find(ik_key);
		if (i_at == ik_at.end()) {
			i_at = ik_at.emplace(ik_key, (uint32_t)ik_leaf.size()).first;
			for (size_t k = 0; k < c.prog.ik_bones.size(); ++k) {
				uint32_t leaf = LMX_BONE_NONE;
				for (uint32_t b = 0; bone_hashes && b < in.n_bones; ++b)
					if (bone_hashes[in.bone_offset + b] == c.prog.ik_leaf_hash[k]) {
						leaf = b;
						break;
					}
				if (leaf != LMX_BONE_NONE) {
					int32_t b = (int32_t)leaf;
					for (uint32_t up = 1; up < c.prog.ik_bones[k]; ++up) {
						b = sk.parents[in.model_offset + (uint32_t)b];
						if (b < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: IK chain of %u bones walks past the root (bone %u has %u ancestors)", i, c.prog.ik_bones[k], leaf, up - 1);
					}
				}
				ik_leaf.push_back(leaf);
			}
		}
		a.ik_off = i_at->second;
		input_types.insert(input_types.end(), c.prog.input_types.begin(), c.prog.input_types.end());
		if (flags[i] & LMX_ANIMATOR_USE_ROOT_MOTION) {
			if (ctx->world.built && (entity[i] < 0 || (uint32_t)entity[i] >= ctx->world.n)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: entity %d out of range", i, entity[i]);
			if (entity[i] < 0) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instance %u: USE_ROOT_MOTION needs an entity", i);
			if (!rm_seen.emplace(entity[i], i).second) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "instances %u and %u move entity %d by root motion", rm_seen[entity[i]], i, entity[i]);
			rm_animator.push_back(i);
			rm_entity.push_back(entity[i]);
		}
	}
	// the lane order: by controller, instances in their own order inside; the runtime-data words of a controller's Animators are columns
	std::vector<uint32_t> group_base(as.controllers.size() + 1, 0), group_lane(as.controllers.size() + 1, 0), taken(as.controllers.size(), 0);
	uint64_t state_words = 0, total_slots = 0;
	for (size_t k = 0; k < as.controllers.size(); ++k) {
		group_base[k] = (uint32_t)state_words;
		group_lane[k + 1] = group_lane[k] + per_controller[k];
		state_words += (uint64_t)per_controller[k] * as.controllers[k].prog.state_words;
		total_slots += (uint64_t)per_controller[k] * as.controllers[k].prog.max_instrs;
	}
	if (state_words > 0x7fffffffull || total_slots > 0x7fffffffull || input_types.size() > 0x3fffffffull) return fail(ctx, LMX_ERR_CAPACITY, "the Animators' state does not fit 32-bit offsets");
	order.resize(group_lane[as.controllers.size()]);
	uint32_t instr_base = 0;
	for (uint32_t i = 0; i < n_instances; ++i) {
		CtlAnimator& a = animators[i];
		a.instr_base = instr_base;
		if (a.controller == LMX_CONTROLLER_NONE) continue;
		const uint32_t k = a.controller, local = taken[k]++;
		order[group_lane[k] + local] = i;
		a.state_base = group_base[k] + local;
		a.state_stride = per_controller[k];
		instr_base += as.controllers[k].prog.max_instrs;
	}
	// the program tables of every controller, concatenated
	std::vector<CtlHeader> headers(as.controllers.size());
	std::vector<CtlNode> nodes;
	std::vector<CtlOp> ops;
	std::vector<uint32_t> exprs, aux;
	for (size_t k = 0; k < as.controllers.size(); ++k) {
		const ControllerProgram& p = as.controllers[k].prog;
		headers[k] = CtlHeader{(uint32_t)nodes.size(), (uint32_t)ops.size(), (uint32_t)exprs.size(), (uint32_t)aux.size(), p.root, (uint32_t)p.input_types.size(), p.state_words, p.max_instrs};
		// (expressions name ops relative to the controller's first)
		nodes.insert(nodes.end(), p.nodes.begin(), p.nodes.end());
		ops.insert(ops.end(), p.ops.begin(), p.ops.end());
		exprs.insert(exprs.end(), p.exprs.begin(), p.exprs.end());
		aux.insert(aux.end(), p.aux.begin(), p.aux.end());
	}
	// every Animator's state is its controller's enter image (Controller::createRuntime), root_motion {0,0,0},{0,0,0,1}, inputs zero and typed
	std::vector<uint32_t> state((size_t)state_words, 0u), state_len(n_instances, 0u), inputs(4 * input_types.size(), 0u);
	std::vector<float> root_motion(7 * (size_t)n_instances, 0.f);
	for (uint32_t i = 0; i < n_instances; ++i) {
		root_motion[7 * (size_t)i + 6] = 1.f;
		const CtlAnimator& a = animators[i];
		if (a.controller == LMX_CONTROLLER_NONE) continue;
		const ControllerProgram& p = as.controllers[a.controller].prog;
		for (size_t w = 0; w < p.enter_image.size(); ++w) state[a.state_base + w * a.state_stride] = p.enter_image[w];
		state_len[i] = (uint32_t)p.enter_image.size();
	}
	for (size_t r = 0; r < input_types.size(); ++r) inputs[4 * r] = input_types[r];
	std::vector<uint32_t> zeros((size_t)n_instances + 1, 0u);
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	LMX_HIP(ctx, upload_blocking(as.d_headers, headers));
	LMX_HIP(ctx, upload_blocking(as.d_nodes, nodes));
	LMX_HIP(ctx, upload_blocking(as.d_ops, ops));
	LMX_HIP(ctx, upload_blocking(as.d_exprs, exprs));
	LMX_HIP(ctx, upload_blocking(as.d_aux, aux));
	LMX_HIP(ctx, upload_blocking(as.d_slots, slots));
	LMX_HIP(ctx, upload_blocking(as.d_ik_leaf, ik_leaf));
	LMX_HIP(ctx, upload_blocking(as.d_order, order));
	LMX_HIP(ctx, upload_blocking(as.d_animators, animators));
	LMX_HIP(ctx, upload_blocking(as.d_inputs, inputs));
	LMX_HIP(ctx, upload_blocking(as.d_input_types, input_types));
	LMX_HIP(ctx, upload_blocking(as.d_state[0], state));
	LMX_HIP(ctx, as.d_state[1].reserve(std::max<size_t>(state.size(), 1)));
	LMX_HIP(ctx, upload_blocking(as.d_state_len, state_len));
	LMX_HIP(ctx, upload_blocking(as.d_counts, zeros));
	LMX_HIP(ctx, upload_blocking(as.d_root_motion, root_motion));
	LMX_HIP(ctx, upload_blocking(as.d_rm_animator, rm_animator));
	LMX_HIP(ctx, upload_blocking(as.d_rm_entity, rm_entity));
	LMX_HIP(ctx, as.d_rm_tr.reserve(std::max<size_t>(rm_entity.size(), 1)));
	LMX_HIP(ctx, as.d_slots_out.reserve(std::max<size_t>((size_t)total_slots, 1)));
	LMX_HIP(ctx, ctx->anim.d_first_sample.reserve((size_t)n_instances + 1));
	LMX_HIP(ctx, upload_blocking(ctx->anim.d_first_sample.p, zeros.data(), zeros.size())); // no update yet: lmx_animators_read_instrs reads empty programs
	LMX_HIP(ctx, ctx->anim.d_instrs.reserve(std::max<size_t>((size_t)total_slots, 1)));
	size_t temp = 0;
	LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n_instances + 1), ctx->stream));
	LMX_HIP(ctx, as.d_scan_temp.reserve(std::max<size_t>(temp, 1)));
	as.animators.swap(animators);
	as.input_types.swap(input_types);
	as.slots_at.swap(slots_at);
	as.rm_entity.swap(rm_entity);
	as.n = n_instances;
	as.n_active = (uint32_t)order.size();
	as.n_rm = (uint32_t)rm_animator.size();
	as.flip = 0;
	as.total_slots = (uint32_t)total_slots;
	as.total_inputs = (uint32_t)as.input_types.size();
	as.any_ik = false;
	for (const CtlAnimator& a : as.animators) as.any_ik = as.any_ik || (a.controller != LMX_CONTROLLER_NONE && !as.controllers[a.controller].prog.ik_bones.empty());
	as.is_set = true;
	return LMX_OK;
}

int lmx_animators_set_inputs(LmxContext* ctx, uint32_t first_animator, uint32_t n, const LmxAnimatorValue* values) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (first_animator > as.n || n > as.n - first_animator) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "Animators [%u, %u + %u) of %u", first_animator, first_animator, n, as.n);
	uint32_t base, count;
	input_range(as, first_animator, n, base, count);
	if (!count) return LMX_OK;
	if (!values) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null values");
	as.inputs_scratch.resize(4 * (size_t)count);
	for (uint32_t r = 0; r < count; ++r) {
		if (values[r].type != as.input_types[base + r]) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "value %u has type %u, the controller declares %u", r, values[r].type, as.input_types[base + r]);
		memcpy(&as.inputs_scratch[4 * (size_t)r], &values[r], 16);
		if (values[r].type == LMX_VALUE_BOOL) as.inputs_scratch[4 * (size_t)r + 1] = values[r].b != 0;
	}
	LMX_HIP(ctx, upload_on_stream(as.d_inputs.p + 4 * (size_t)base, as.inputs_scratch.data(), as.inputs_scratch.size(), ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the scratch array is pageable and reused
	return LMX_OK;
}

int lmx_animators_set_inputs_device(LmxContext* ctx, uint32_t first_animator, uint32_t n, const void* d_values) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (first_animator > as.n || n > as.n - first_animator) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "Animators [%u, %u + %u) of %u", first_animator, first_animator, n, as.n);
	uint32_t base, count;
	input_range(as, first_animator, n, base, count);
	if (!count) return LMX_OK;
	if (!d_values) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "null device pointer");
	LMX_HIP(ctx, launch_animators_set_inputs(ctx->stream, (const uint32_t*)d_values, as.d_input_types.p + base, as.d_inputs.p + 4 * (size_t)base, count));
	return LMX_OK;
}

int lmx_animators_update(LmxContext* ctx, float time_delta) {
	LMX_CHECK_CTX(ctx);
	SkinState& sk = ctx->skin;
	AnimState& an = ctx->anim;
	AnimatorsState& as = ctx->animators;
	// lmx_anim_update's rules, and Time::fromSeconds asserts time >= 0 (animation.h:21)
	if (!std::isfinite(time_delta) || !(time_delta >= 0.f) || !(time_delta * (float)LMX_TIME_ONE_SECOND < 4294967296.f))
		return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "time_delta %g: not finite, negative, or more than 2^32 ticks of 1 / %u s", (double)time_delta, LMX_TIME_ONE_SECOND);
	if (!as.is_set || as.n != sk.inst.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called for this instance table");
	if (!as.n) return LMX_OK;
	if (an.rel_rot.size() != sk.parents.size()) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_anim_set_model_pose is missing for a model added later");
	if (int rc = anim_upload_tables(ctx)) return rc;
	if (int rc = upload_clips(ctx)) return rc;
	if (an.parents_uploaded != sk.parents.size()) { // evalIK's chain walk; models only append
		LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
		LMX_HIP(ctx, upload_blocking(an.d_parents, sk.parents.data(), sk.parents.size()));
		an.parents_uploaded = sk.parents.size();
	}
	Grow grow{ctx}; // (the buffers are shared with lmx_anim_eval_blend_*: a call there may have come first, or none)
	if (int rc = grow(an.d_first_sample, (size_t)as.n + 1)) return rc;
	if (int rc = grow(an.d_instrs, std::max<size_t>(as.total_slots, 1))) return rc;
	if (int rc = grow(an.d_samples, std::max<size_t>(as.total_slots, 1))) return rc;
	AnimatorTables at;
	at.headers = as.d_headers.p; at.nodes = as.d_nodes.p; at.ops = as.d_ops.p; at.exprs = as.d_exprs.p; at.aux = as.d_aux.p; at.slots = as.d_slots.p;
	at.ik_leaf = as.d_ik_leaf.p; at.clips = as.d_clips.p; at.rm_t = as.d_rm_t.p; at.rm_r = as.d_rm_r.p;
	AnimTables t;
	t.src = an.d_src.p; t.const_translations = an.d_ct.p; t.translations = an.d_tt.p; t.const_rotations = an.d_cr.p; t.rotations = an.d_rt.p;
	t.translation_stream = an.d_tstream.p; t.rotation_stream = an.d_rstream.p; t.root_translations = an.d_root_t.p; t.root_rotations = an.d_root_r.p;
	{
	ProfScope ps(ctx, LMX_K_ANIMATORS_UPDATE);
	LMX_HIP(ctx, launch_animators_update(ctx->stream, at, as.d_animators.p, as.d_order.p, as.n_active, as.d_inputs.p, as.d_state[as.flip].p, as.d_state[as.flip ^ 1].p,
		as.d_state_len.p, as.d_root_motion.p, as.d_slots_out.p, as.d_counts.p, time_from_seconds(time_delta)));
	}
	as.flip ^= 1; // the kernel is enqueued: the new stream is the state from here on
	{
	ProfScope ps(ctx, LMX_K_ANIMATORS_PACK);
	size_t temp = as.d_scan_temp.cap;
	LMX_HIP(ctx, hipcub::DeviceScan::ExclusiveSum(as.d_scan_temp.p, temp, as.d_counts.p, an.d_first_sample.p, (int)(as.n + 1), ctx->stream));
	LMX_HIP(ctx, launch_animators_pack(ctx->stream, as.d_animators.p, as.n, an.d_first_sample.p, as.d_counts.p, as.d_slots_out.p, an.d_instrs.p, as.any_ik ? nullptr : an.d_samples.p));
	}
	ProfScope ps(ctx, LMX_K_ANIM_UPDATE);
	if (as.any_ik)
		LMX_HIP(ctx, launch_anim_blend_instrs(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, (uint32_t)an.anims.size(), an.d_instrs.p,
			an.d_first_sample.p, an.d_parents.p, an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	else // as lmx_anim_eval_blend_instrs does for a call without IK: k_anim_blend_stack on the SAMPLE fields
		LMX_HIP(ctx, launch_anim_blend_stack(ctx->stream, sk.d_inst.p, (uint32_t)sk.inst.size(), an.d_anims.p, t, (uint32_t)an.anims.size(), an.d_samples.p,
			an.d_first_sample.p, an.d_rel_pos.p, an.d_rel_rot.p, sk.d_pose_pos.p, sk.d_pose_rot.p));
	sk.borrowed_pos = nullptr;
	sk.borrowed_rot = nullptr;
	sk.poses_uploaded = true;
	sk.pose_is_absolute = false;
	return LMX_OK;
}

int lmx_animators_read_root_motion(LmxContext* ctx, LmxLocalRigidTransform* out, uint32_t n_animators) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (n_animators != as.n || (n_animators && !out)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "expected %u Animators", as.n);
	return read_now(ctx, (float*)out, (const float*)as.d_root_motion.p, 7 * (size_t)n_animators);
}

int lmx_animators_device_outputs(LmxContext* ctx, void** d_root_motion, void** d_first_instr, void** d_instrs) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (d_root_motion) *d_root_motion = as.d_root_motion.p;
	if (d_first_instr) *d_first_instr = ctx->anim.d_first_sample.p;
	if (d_instrs) *d_instrs = ctx->anim.d_instrs.p;
	return LMX_OK;
}

int lmx_animators_apply_root_motion(LmxContext* ctx) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	WorldState& w = ctx->world;
	if (!w.built) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_world_build has not been called");
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (!as.n_rm) return LMX_OK;
	for (int32_t e : as.rm_entity) // (lmx_animators_set may have run before the world was built)
		if ((uint32_t)e >= w.n) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "root-motion entity %d out of range", e);
	if (w.n_live != w.n)
		for (int32_t e : as.rm_entity)
			if (!w.mirror.alive(e)) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "root-motion entity %d was destroyed", e);
	w.pending = true; // staged like lmx_world_set_world_transforms: lmx_world_edit propagates first
	LMX_HIP(ctx, launch_animators_root_motion(ctx->stream, w.dev(), w.d_slot_of_entity.p, as.d_rm_animator.p, as.d_rm_entity.p, as.n_rm, as.d_root_motion.p, as.d_rm_tr.p));
	// World::setTransform (animation_module.cpp:634): the path of lmx_world_set_world_transforms, fed from device memory
	LMX_HIP(ctx, launch_xform_scatter(ctx->stream, w.dev(), w.d_slot_of_entity.p, as.d_rm_entity.p, as.d_rm_tr.p, as.n_rm, XF_STAGE_SET_WORLD));
	return LMX_OK;
}

int lmx_animators_read_state(LmxContext* ctx, uint32_t animator, void* out, uint32_t capacity_bytes, uint32_t* out_bytes) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (animator >= as.n || !out_bytes) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "bad Animator / null out_bytes");
	const CtlAnimator& a = as.animators[animator];
	*out_bytes = 0;
	if (a.controller == LMX_CONTROLLER_NONE) return LMX_OK;
	uint32_t len = 0;
	if (int rc = read_now(ctx, &len, (const uint32_t*)as.d_state_len.p + animator, 1)) return rc;
	*out_bytes = 4 * len;
	if (!out) return LMX_OK;
	if (capacity_bytes < 4 * len) return fail(ctx, LMX_ERR_CAPACITY, "need room for %u bytes", 4 * len);
	for (uint32_t k = 0; k < len; ++k) // a column of the state, word by word: a read-out for tests and tools
		LMX_HIP(ctx, read_back((uint32_t*)out + k, as.d_state[as.flip].p + a.state_base + (size_t)k * a.state_stride, 1, ctx->stream));
	LMX_HIP(ctx, hipStreamSynchronize(ctx->stream));
	return LMX_OK;
}

int lmx_animators_read_instrs(LmxContext* ctx, uint32_t* out_first_instr, uint32_t n_animators, LmxBlendInstr* out_instrs, uint32_t capacity, uint32_t* out_count) {
	LMX_CHECK_CTX(ctx);
	AnimatorsState& as = ctx->animators;
	if (!as.is_set) return fail(ctx, LMX_ERR_NOT_BUILT, "lmx_animators_set has not been called");
	if (n_animators != as.n || !out_first_instr || !out_count) return fail(ctx, LMX_ERR_INVALID_ARGUMENT, "expected %u Animators and non-null outputs", as.n);
	if (int rc = read_now(ctx, out_first_instr, (const uint32_t*)ctx->anim.d_first_sample.p, (size_t)as.n + 1)) return rc;
	const uint32_t total = out_first_instr[as.n];
	*out_count = total;
	if (!out_instrs) return LMX_OK;
	return read_out(ctx, out_instrs, capacity, (const LmxBlendInstr*)ctx->anim.d_instrs.p, total, total, "instructions");
}

} // extern "C"
