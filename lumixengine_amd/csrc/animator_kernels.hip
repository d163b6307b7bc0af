// animator_kernels.hip — AnimationModuleImpl::updateAnimator's first half on gfx950 (animation_module.cpp:602-636): Controller::update
// (controller.cpp:69-79) of every Animator, the hand-off of its blend instructions to the blend kernels of anim_kernels.hip, and its root motion into the world.
//
// One lane per Animator runs the VM of lmx_controller_program.h - the same statements the host runs for a controller's enter image.
// Animators are ordered by controller, so a wave mostly shares one program and its loads of node records are uniform; the runtime-data
// words of a controller's Animators are stored as columns (word k of 64 neighbouring Animators is one 256-byte line). The VM's explicit
// stacks (LMX_CONTROLLER_MAX_POSE_DEPTH frames of 48 bytes, the value operands, the skip list) are indexed at run time and live in scratch:
// 400 bytes a lane, touched only by nodes that nest, and a frame of animation runs this kernel once per Animator against the blend
// kernel's 64 lanes per Animator.
#include "lmx_kernels.h"

namespace lmx {

namespace {

__global__ __launch_bounds__(64) void k_animators_update(AnimatorTables t, const CtlAnimator* __restrict__ animators, const uint32_t* __restrict__ order, uint32_t n_active,
	const uint32_t* __restrict__ inputs, const uint32_t* __restrict__ state_in, uint32_t* __restrict__ state_out, uint32_t* __restrict__ state_len,
	float* __restrict__ root_motion, LmxBlendInstr* __restrict__ slots_out, uint32_t* __restrict__ counts, uint32_t time_delta) {
	const uint32_t p = blockIdx.x * 64u + threadIdx.x;
	if (p >= n_active) return;
	const uint32_t a = order[p];
	const CtlAnimator an = animators[a];
	const CtlHeader h = t.headers[an.controller];
	CtlCtx c;
	c.nodes = t.nodes + h.nodes_off;
	c.ops = t.ops + h.ops_off;
	c.exprs = t.exprs + h.exprs_off;
	c.aux = t.aux + h.aux_off;
	c.slots = t.slots + an.slots_off;
	c.clips = t.clips;
	c.rm_t = t.rm_t;
	c.rm_r = t.rm_r;
	c.inputs = inputs + 4 * (size_t)an.input_base;
	c.ik_leaf = t.ik_leaf + an.ik_off;
	c.in = state_in + an.state_base;
	c.out = state_out + an.state_base;
	c.stride = an.state_stride;
	c.rd = 0;
	c.wr = 0;
	c.time_delta = time_delta;
	c.weight = 1.f;
	float* rm = root_motion + 7 * (size_t)a;
	c.root_motion = Rigid{V3{rm[0], rm[1], rm[2]}, Q4{rm[3], rm[4], rm[5], rm[6]}}; // a BLEND2D early return leaves last frame's value standing
	c.instrs = slots_out + an.instr_base;
	c.n_instrs = 0;
	CtlFrame stack[LMX_CONTROLLER_MAX_POSE_DEPTH];
	ctl_update(c, h.root, stack);
	state_len[a] = c.wr;
	counts[a] = c.n_instrs;
	rm[0] = c.root_motion.pos.x; rm[1] = c.root_motion.pos.y; rm[2] = c.root_motion.pos.z;
	rm[3] = c.root_motion.rot.x; rm[4] = c.root_motion.rot.y; rm[5] = c.root_motion.rot.z; rm[6] = c.root_motion.rot.w;
}

__global__ __launch_bounds__(256) void k_animators_pack(const CtlAnimator* __restrict__ animators, uint32_t n, const uint32_t* __restrict__ first,
	const uint32_t* __restrict__ counts, const LmxBlendInstr* __restrict__ slots_out, LmxBlendInstr* __restrict__ packed, LmxBlendSample* __restrict__ samples) {
	const uint32_t a = blockIdx.x * 256u + threadIdx.x;
	if (a >= n) return;
	const uint32_t k = counts[a];
	const uint4* src = (const uint4*)(slots_out + animators[a].instr_base);
	uint4* dst = (uint4*)(packed + first[a]);
	for (uint32_t i = 0; i < 3 * k; ++i) dst[i] = src[i]; // 48-byte records
	if (!samples) return;
	for (uint32_t i = 0; i < k; ++i) { // no controller in use has an IK node: the records' SAMPLE fields in k_anim_blend_stack's 16-byte form
		const uint4 head = src[3 * i];       // op, animation, weight, time
		const uint32_t looped = ((const uint32_t*)(src + 3 * i + 1))[0];
		((uint4*)samples)[first[a] + i] = make_uint4(head.y, head.z, head.w, looped);
	}
}

__global__ __launch_bounds__(256) void k_animators_set_inputs(const uint32_t* __restrict__ values, const uint32_t* __restrict__ types, uint32_t* __restrict__ inputs,
	uint32_t n_records) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n_records) return;
	const uint4 v = ((const uint4*)values)[i];
	const uint32_t type = types[i];
	((uint4*)inputs)[i] = make_uint4(type, type == LMX_VALUE_BOOL ? (uint32_t)((v.y & 0xffu) != 0) : v.y, v.z, v.w);
}

struct RootMotionTransform { double pos[3]; float rot[4]; float scale[3]; float pad; }; // LmxTransform

__global__ __launch_bounds__(256) void k_animators_root_motion(WorldDevice w, const int32_t* __restrict__ slot_of_entity, const uint32_t* __restrict__ animator,
	const int32_t* __restrict__ entity, uint32_t n, const float* __restrict__ root_motion, RootMotionTransform* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const int32_t s = slot_of_entity[entity[i]];
	const float* rm = root_motion + 7 * (size_t)animator[i];
	const float4 wr = w.wrot[s];
	const Q4 rot = Q4{wr.x, wr.y, wr.z, wr.w};
	const DV3 pos = add(DV3{w.wpx[s], w.wpy[s], w.wpz[s]}, rotate(rot, V3{rm[0], rm[1], rm[2]})); // tr.pos += tr.rot.rotate(root_motion.pos)
	const Q4 r = qmul(Q4{rm[3], rm[4], rm[5], rm[6]}, rot);                                      // tr.rot = root_motion.rot * tr.rot
	RootMotionTransform o;
	o.pos[0] = pos.x; o.pos[1] = pos.y; o.pos[2] = pos.z;
	o.rot[0] = r.x; o.rot[1] = r.y; o.rot[2] = r.z; o.rot[3] = r.w;
	o.scale[0] = w.wsx[s]; o.scale[1] = w.wsy[s]; o.scale[2] = w.wsz[s];
	o.pad = 0.f;
	out[i] = o;
}

} // namespace

hipError_t launch_animators_update(hipStream_t s, const AnimatorTables& t, const CtlAnimator* animators, const uint32_t* order, uint32_t n_active, const uint32_t* inputs,
	const uint32_t* state_in, uint32_t* state_out, uint32_t* state_len, float* root_motion, LmxBlendInstr* slots_out, uint32_t* counts, uint32_t time_delta) {
	if (!n_active) return hipSuccess;
	hipLaunchKernelGGL(k_animators_update, dim3((n_active + 63u) / 64u), dim3(64), 0, s, t, animators, order, n_active, inputs, state_in, state_out, state_len, root_motion,
		slots_out, counts, time_delta);
	return hipGetLastError();
}

hipError_t launch_animators_pack(hipStream_t s, const CtlAnimator* animators, uint32_t n, const uint32_t* first, const uint32_t* counts, const LmxBlendInstr* slots_out,
	LmxBlendInstr* packed, LmxBlendSample* samples) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_animators_pack, dim3((n + 255u) / 256u), dim3(256), 0, s, animators, n, first, counts, slots_out, packed, samples);
	return hipGetLastError();
}

hipError_t launch_animators_set_inputs(hipStream_t s, const uint32_t* values, const uint32_t* types, uint32_t* inputs, uint32_t n_records) {
	if (!n_records) return hipSuccess;
	hipLaunchKernelGGL(k_animators_set_inputs, dim3((n_records + 255u) / 256u), dim3(256), 0, s, values, types, inputs, n_records);
	return hipGetLastError();
}

hipError_t launch_animators_root_motion(hipStream_t s, const WorldDevice& w, const int32_t* slot_of_entity, const uint32_t* animator, const int32_t* entity, uint32_t n,
	const float* root_motion, void* out) {
	if (!n) return hipSuccess;
	hipLaunchKernelGGL(k_animators_root_motion, dim3((n + 255u) / 256u), dim3(256), 0, s, w, slot_of_entity, animator, entity, n, root_motion, (RootMotionTransform*)out);
	return hipGetLastError();
}

} // namespace lmx
