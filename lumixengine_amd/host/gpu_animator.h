// gpu_animator.h — the evalBlendStack stand-in of AnimationModuleImpl::updateAnimator (C++ host side of include/lumix_mi355.h
// "animation": lmx_anim_decode_blend_stack / lmx_anim_eval_blend_instrs).
//
// In the reference updateAnimator (src/animation/animation_module.cpp:602-636) runs Controller::update(ctx, root_motion), which leaves the
// frame's instructions in ctx->blendstack, then Model::getRelativePose + evalBlendStack(ctx, pose) + Pose::computeAbsolute per Animator.
// The node graph stays where it is; GpuAnimators takes the pose work: per frame begin(), then for every skin instance in table order
// add(ctx) with the Animator's RuntimeContext after Controller::update (or addNone() for an instance without an Animator), then eval():
// one lmx_anim_eval_blend_instrs call for all of them - SAMPLE and IK instructions alike - and lmx_skin_run does computeAbsolute and the
// palette. Root motion (:630-635) comes from the CPU node graph and goes through the engine's own setters.
//
// setAnimation() tells which library id (lmx_anim_add) an Animation resource has; bone name hashes are taken from Model::getBones()[i].name
// as Model::parse hashes them (BoneNameHash(name.c_str()), renderer/model.cpp:361) and cached per model.
//
// `Context` is anim::RuntimeContext inside the engine (-DLMX_WITH_LUMIX_HEADERS); a standalone build passes any type with blendstack,
// animations, weight and model (tests/cpp/lumix_compat_animator.h).
#pragma once

#include <utility>
#include <vector>

#include "lumix_mi355.h"

#ifdef LMX_WITH_LUMIX_HEADERS
	#include "animation/animation.h"
	#include "animation/controller.h"
	#include "core/hash.h"
	#include "renderer/model.h"
#else
	#include "lumix_compat.h"
	#include "lumix_compat_animator.h"
#endif

namespace Lumix {

struct GpuAnimators {
	explicit GpuAnimators(LmxContext* ctx) : m_ctx(ctx) {}
	GpuAnimators(const GpuAnimators&) = delete;
	void operator=(const GpuAnimators&) = delete;

	// `id`: what lmx_anim_add returned for this Animation resource
	void setAnimation(const void* animation, u32 id) {
		for (auto& a : m_animations)
			if (a.first == animation) { a.second = id; return; }
		m_animations.push_back(std::make_pair(animation, id));
	}

	void begin() {
		m_first.clear();
		m_first.push_back(0);
		m_instrs.clear();
	}

	// The next skin instance's Animator, after Controller::update(ctx, root_motion). False: the blend stack is malformed or names an
	// animation that was never registered - the instance gets an empty program (its model's relative pose) and the engine should run
	// evalBlendStack for it itself.
	template <typename Context> bool add(const Context& ctx) {
		const size_t at = m_instrs.size();
		bool ok = ctx.model != nullptr;
		if (ok) {
			m_slots.clear();
			for (const auto* animation : ctx.animations) m_slots.push_back(idOf(animation));
			const std::vector<u64>& hashes = hashesOf(*ctx.model);
			const u64 size = ctx.blendstack.size();
			m_instrs.resize(at + (size_t)size); // an instruction takes at least one byte: never too small
			u32 count = 0;
			ok = lmx_anim_decode_blend_stack((const uint8_t*)ctx.blendstack.data(), size, m_slots.data(), (u32)m_slots.size(), hashes.data(), (u32)hashes.size(), ctx.weight,
					 m_instrs.data() + at, (u32)size, &count) == LMX_OK;
			m_instrs.resize(at + (ok ? count : 0));
		}
		m_first.push_back((u32)m_instrs.size());
		return ok;
	}

	// a skin instance without an Animator: it keeps its model's relative pose
	void addNone() { m_first.push_back((u32)m_instrs.size()); }

	// evalBlendStack of every instance added since begin(): enqueues and returns. lmx_skin_run follows.
	bool eval() { return lmx_anim_eval_blend_instrs(m_ctx, (u32)m_first.size() - 1, m_first.data(), m_instrs.data()) == LMX_OK; }

	u32 instructionCount() const { return (u32)m_instrs.size(); }
	const char* lastError() const { return lmx_last_error(m_ctx); }

private:
	u32 idOf(const void* animation) const {
		for (const auto& a : m_animations)
			if (a.first == animation) return a.second;
		return LMX_ANIM_NONE;
	}

	template <typename ModelT> const std::vector<u64>& hashesOf(const ModelT& model) {
		for (const auto& m : m_models)
			if (m.first == (const void*)&model) return m.second;
		std::vector<u64> hashes;
		for (const auto& bone : model.getBones()) hashes.push_back(BoneNameHash(bone.name.c_str()).getHashValue());
		m_models.push_back(std::make_pair((const void*)&model, std::move(hashes)));
		return m_models.back().second;
	}

	LmxContext* m_ctx;
	std::vector<std::pair<const void*, u32>> m_animations;
	std::vector<std::pair<const void*, std::vector<u64>>> m_models;
	std::vector<u32> m_slots;
	std::vector<u32> m_first;
	std::vector<LmxBlendInstr> m_instrs;
};

// The whole first half of updateAnimator on the device (include/lumix_mi355.h "animator controllers"): Controller::update runs there too, so
// nothing of an Animator crosses the bus per frame but the inputs that changed. GpuAnimators above stays for engines that keep the node graph.
//   setController(resource bytes) once per anim::Controller resource (the bytes Controller::load receives), setSlots(controller, set, ids)
//   once per animation set (ids: lmx_anim_add's, LMX_ANIM_NONE for an empty slot), setAnimators(...) once per skin instance table;
//   per frame setInput(animator, idx, value) for what changed (RuntimeContext::setInput), update(time_delta) - Controller::update +
//   evalBlendStack of every Animator; lmx_skin_run follows - and rootMotion(i), or lmx_animators_apply_root_motion + lmx_world_propagate
//   for the Animators with USE_ROOT_MOTION.
struct GpuAnimatorControllers {
	explicit GpuAnimatorControllers(LmxContext* ctx) : m_ctx(ctx) {}
	GpuAnimatorControllers(const GpuAnimatorControllers&) = delete;
	void operator=(const GpuAnimatorControllers&) = delete;

	// LMX_CONTROLLER_NONE: the resource is malformed or uses what the library refuses (lastError() says what)
	u32 setController(const void* bytes, u64 size) {
		u32 id = LMX_CONTROLLER_NONE, count = 0;
		if (lmx_anim_controller_add(m_ctx, bytes, size, &id) != LMX_OK) return LMX_CONTROLLER_NONE;
		if (m_types_of.size() <= id) m_types_of.resize(id + 1);
		if (lmx_anim_controller_input_types(m_ctx, id, nullptr, 0, &count) != LMX_OK) return LMX_CONTROLLER_NONE;
		m_types_of[id].resize(count);
		if (count && lmx_anim_controller_input_types(m_ctx, id, m_types_of[id].data(), count, &count) != LMX_OK) return LMX_CONTROLLER_NONE;
		return id;
	}

	bool setSlots(u32 controller, u32 set, const u32* animation_ids, u32 n_slots) { return lmx_anim_controller_set_slots(m_ctx, controller, set, animation_ids, n_slots) == LMX_OK; }

	// one entry per skin instance, in table order; bone_hashes: every instance's bone name hashes back to back (Model::getBones()[i].name hashed)
	bool setAnimators(u32 n, const u32* controller, const u32* set, const u32* flags, const i32* entity, const u64* bone_hashes, u32 n_bone_hashes) {
		if (lmx_animators_set(m_ctx, n, controller, set, flags, entity, bone_hashes, n_bone_hashes) != LMX_OK) return false;
		m_first.assign(n + 1, 0);
		for (u32 i = 0; i < n; ++i) m_first[i + 1] = m_first[i] + (controller[i] == LMX_CONTROLLER_NONE ? 0 : (u32)m_types_of[controller[i]].size());
		m_values.assign(m_first[n], LmxAnimatorValue{});
		for (u32 i = 0; i < n; ++i) // Controller::createRuntime, controller.cpp:53-57: every input zero and typed - an Animator between two changed ones is uploaded as it is
			for (u32 k = m_first[i]; k < m_first[i + 1]; ++k) m_values[k].type = m_types_of[controller[i]][k - m_first[i]];
		m_dirty_lo = n;
		m_dirty_hi = 0;
		m_root_motion.assign(n, LmxLocalRigidTransform{{0, 0, 0}, {0, 0, 0, 1}});
		m_root_motion_read = true;
		return true;
	}

	// RuntimeContext::setInput, controller.h:42-43 (and a Vec3, which the IK node's effector reads)
	void setInput(u32 animator, u32 idx, float value) { LmxAnimatorValue v{}; v.type = LMX_VALUE_NUMBER; v.f = value; put(animator, idx, v); }
	void setInput(u32 animator, u32 idx, bool value) { LmxAnimatorValue v{}; v.type = LMX_VALUE_BOOL; v.b = value ? 1 : 0; put(animator, idx, v); }
	void setInput(u32 animator, u32 idx, const Vec3& value) { LmxAnimatorValue v{}; v.type = LMX_VALUE_VEC3; v.v3[0] = value.x; v.v3[1] = value.y; v.v3[2] = value.z; put(animator, idx, v); }

	// Controller::update + evalBlendStack of every Animator: enqueues and returns. False: time_delta is refused (lastError() says why).
	bool update(float time_delta) {
		if (m_dirty_lo <= m_dirty_hi && m_first.size() > 1) { // one upload: the Animators from the first changed one to the last
			if (lmx_animators_set_inputs(m_ctx, m_dirty_lo, m_dirty_hi - m_dirty_lo + 1, m_values.data() + m_first[m_dirty_lo]) != LMX_OK) return false;
			m_dirty_lo = (u32)m_first.size() - 1;
			m_dirty_hi = 0;
		}
		m_root_motion_read = false;
		return lmx_animators_update(m_ctx, time_delta) == LMX_OK;
	}

	// Animator::root_motion after the last update (animation_module.cpp:621); the first call after an update waits for it
	LocalRigidTransform rootMotion(u32 animator) {
		if (!m_root_motion_read) m_root_motion_read = lmx_animators_read_root_motion(m_ctx, m_root_motion.data(), (u32)m_root_motion.size()) == LMX_OK;
		const LmxLocalRigidTransform& r = m_root_motion[animator];
		LocalRigidTransform out;
		out.pos.x = r.pos[0]; out.pos.y = r.pos[1]; out.pos.z = r.pos[2];
		out.rot.x = r.rot[0]; out.rot.y = r.rot[1]; out.rot.z = r.rot[2]; out.rot.w = r.rot[3];
		return out;
	}

	bool applyRootMotion() { return lmx_animators_apply_root_motion(m_ctx) == LMX_OK; }
	const char* lastError() const { return lmx_last_error(m_ctx); }

private:
	// an input that does not exist, or of another type than the controller declares (RuntimeContext::setInput asserts it), is left as it is
	void put(u32 animator, u32 idx, const LmxAnimatorValue& v) {
		if (animator + 1 >= m_first.size() || idx >= m_first[animator + 1] - m_first[animator]) return;
		if (m_values[m_first[animator] + idx].type != v.type) return;
		m_values[m_first[animator] + idx] = v;
		if (animator < m_dirty_lo) m_dirty_lo = animator;
		if (animator > m_dirty_hi) m_dirty_hi = animator;
	}

	LmxContext* m_ctx;
	std::vector<std::vector<u32>> m_types_of; // per controller: Controller::m_inputs[i].type
	std::vector<u32> m_first;     // per Animator: its first input record
	std::vector<LmxAnimatorValue> m_values;
	std::vector<LmxLocalRigidTransform> m_root_motion;
	u32 m_dirty_lo = 0, m_dirty_hi = 0;
	bool m_root_motion_read = true;
};

} // namespace Lumix
