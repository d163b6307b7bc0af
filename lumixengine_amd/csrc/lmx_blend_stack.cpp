// lmx_blend_stack.cpp — evalBlendStack's reader (animation/controller.cpp:267-293) turned into a decoder: the bytes the controller's
// nodes wrote (SAMPLE: nodes.cpp, IK: IKNode::update nodes.cpp:357-369) become LmxBlendInstr records for lmx_anim_eval_blend_instrs.
// Every read is checked against the end of the stream; nothing is allocated.
#include <cstring>

#include "lmx_blend_stack.h"
#include "lumix_mi355.h"

namespace lmx {

namespace {

struct Reader {
	const uint8_t* p;
	uint64_t size, pos;
	bool ok;
	template <typename T> T read() {
		T v{};
		if (!ok || size - pos < sizeof(T)) { ok = false; return v; }
		memcpy(&v, p + pos, sizeof(T));
		pos += sizeof(T);
		return v;
	}
};

} // namespace

BlendDecodeResult blend_stack_decode(const uint8_t* bytes, uint64_t n_bytes, const uint32_t* slot_animation, uint32_t n_slots, const uint64_t* bone_hashes,
	uint32_t n_bones, float weight, LmxBlendInstr* out, uint32_t capacity, uint32_t* out_count) {
	Reader r{bytes, n_bytes, 0, true};
	uint32_t n = 0;
	*out_count = 0;
	for (;;) {
		const uint8_t op = r.read<uint8_t>();
		if (!r.ok) return BD_INVALID; // no END
		if (op == 0) break;
		LmxBlendInstr ins;
		memset(&ins, 0, sizeof(ins));
		ins.leaf_bone = LMX_BONE_NONE;
		if (op == LMX_BLEND_SAMPLE) {
			const uint32_t slot = r.read<uint32_t>();
			ins.weight = r.read<float>();
			ins.time = r.read<uint32_t>();
			ins.looped = r.read<uint8_t>() ? 1u : 0u;
			if (!r.ok) return BD_INVALID;
			if (slot >= n_slots || slot_animation[slot] == LMX_ANIM_NONE) return BD_INVALID; // getPose asserts the slot's animation
			ins.op = LMX_BLEND_SAMPLE;
			ins.animation = slot_animation[slot];
		} else if (op == LMX_BLEND_IK) {
			const float alpha = r.read<float>();
			for (int k = 0; k < 3; ++k) ins.target[k] = r.read<float>();
			const uint64_t leaf = r.read<uint64_t>();
			ins.bones_count = r.read<uint32_t>();
			if (!r.ok) return BD_INVALID;
			ins.op = LMX_BLEND_IK;
			ins.alpha = alpha * weight; // controller.cpp:280
			for (uint32_t b = 0; b < n_bones; ++b)
				if (bone_hashes[b] == leaf) { ins.leaf_bone = b; break; }
		} else return BD_INVALID;
		if (n >= capacity) return BD_CAPACITY;
		out[n++] = ins;
		*out_count = n;
	}
	return BD_OK;
}

} // namespace lmx

extern "C" int lmx_anim_decode_blend_stack(const uint8_t* bytes, uint64_t n_bytes, const uint32_t* slot_animation, uint32_t n_slots, const uint64_t* bone_hashes,
	uint32_t n_bones, float weight, LmxBlendInstr* out_instrs, uint32_t capacity, uint32_t* out_count) {
	if (!out_count || (n_bytes && !bytes) || (n_slots && !slot_animation) || (n_bones && !bone_hashes) || (capacity && !out_instrs)) return LMX_ERR_INVALID_ARGUMENT;
	switch (lmx::blend_stack_decode(bytes, n_bytes, slot_animation, n_slots, bone_hashes, n_bones, weight, out_instrs, capacity, out_count)) {
		case lmx::BD_OK: return LMX_OK;
		case lmx::BD_CAPACITY: return LMX_ERR_CAPACITY;
		default: return LMX_ERR_INVALID;
	}
}
