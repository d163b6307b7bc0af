// lmx_blend_stack.h — decoder of an Animator's blend stack bytes (anim::RuntimeContext::blendstack, animation/controller.cpp:267-293)
// into LmxBlendInstr records. Plain C++, no device, no allocation: lmx_blend_stack.cpp, also built on its own by the decoder's tests.
#pragma once

#include <stdint.h>

#include "lmx_types.h"

namespace lmx {

enum BlendDecodeResult : int { BD_OK = 0, BD_INVALID = 1, BD_CAPACITY = 2 };

// `out` may be null when capacity is 0. *out_count: the records written (BD_OK), or decoded so far (otherwise).
BlendDecodeResult blend_stack_decode(const uint8_t* bytes, uint64_t n_bytes, const uint32_t* slot_animation, uint32_t n_slots, const uint64_t* bone_hashes,
	uint32_t n_bones, float weight, LmxBlendInstr* out, uint32_t capacity, uint32_t* out_count);

} // namespace lmx
