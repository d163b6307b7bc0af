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

} // namespace Lumix
