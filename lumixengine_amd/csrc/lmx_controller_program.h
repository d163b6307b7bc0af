// lmx_controller_program.h — an animation controller (anim::Controller, animation/controller.cpp + animation/nodes.cpp) as the
// kernels of animator_kernels.hip run it: the node tree flattened ONCE on the host (lmx_controller_program.cpp, plain C++) into
// fixed-size records, every value tree into a postfix expression, and one VM for Controller::update / PoseNode::enter / skip /
// ValueNode::eval, stated here once for host and device. The VM is non-recursive and carries no checks: every index a record holds
// was validated by controller_program_parse, every nesting depth fits the explicit stacks (LMX_CONTROLLER_MAX_POSE_DEPTH /
// LMX_CONTROLLER_MAX_VALUE_DEPTH, include/lmx_types.h).
//
// Arithmetic is the reference's, operation for operation (no contraction: every user is built with -ffp-contract=off). Conversions the
// reference leaves undefined are DEFINED here as what its x86-64 build does: a float or double to u32 goes through a 64-bit integer
// and keeps the low 32 bits (0 for NaN and outside +-2^63); a float to i32 outside the type's range or NaN gives INT32_MIN.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "lmx_math.h"
#include "lmx_types.h"

namespace lmx {

// anim::NodeType, in the engine's order (animation/nodes.h:22-48)
enum CtlNodeType : uint32_t {
	CN_ANIMATION, CN_BLEND1D, CN_LAYERS, CN_NONE, CN_SELECT, CN_BLEND2D, CN_TREE, CN_OUTPUT, CN_INPUT, CN_SWITCH, CN_CMP_EQ, CN_CMP_NEQ, CN_CMP_LT, CN_CMP_GT,
	CN_CMP_LTE, CN_CMP_GTE, CN_MUL, CN_DIV, CN_ADD, CN_SUB, CN_CONSTANT, CN_AND, CN_OR, CN_PLAYRATE, CN_IK, CN_TYPE_COUNT
};
constexpr uint32_t CTL_ANIMATION_LOOPED = 1u; // AnimationNode::LOOPED

// One pose node. `w` by type (expr: an index into the expression table; node: into the node table; off: into `aux`):
//   ANIMATION  w0 slot, w1 flags
//   BLEND1D    w0 children off ({value, slot} pairs), w1 children, w2 expr
//   BLEND2D    w0 children off ({x, y, slot}), w1 children, w2 triangles off ({a, b, c}), w3 triangles, w4 x expr, w5 y expr
//   SELECT     w0 blend length, w1 children off (nodes), w2 children, w3 expr
//   SWITCH     w0 blend length, w1 true node, w2 false node, w3 expr
//   PLAYRATE   w0 expr, w1 node
//   IK         w0 bones_count, w1 its ordinal among the controller's IK nodes (the per-model leaf table), w2 alpha expr, w3 effector expr, w4 node
struct CtlNode {
	uint32_t type;
	uint32_t w[7];
};
static_assert(sizeof(CtlNode) == 32, "two 16-byte loads");

// One step of a value tree in postfix order. INPUT: a = the input; CONSTANT: a, b, c = the Value's union (a BOOL as 0 / 1); a math node
// pops two words and pushes one. A value is the first word of its union; only an expression of one step can be a VEC3.
struct CtlOp {
	uint32_t op, a, b, c;
};

struct CtlClip { // what the VM reads of an Animation
	float fps;
	uint32_t frame_count, length;
	uint32_t rm_t, rm_r; // first entry of Animation::RootMotion::translations / rotations (frame_count + 1 entries), LMX_ANIM_NONE: empty
};

struct CtlFrame { // a pose node waiting for a child's update
	uint32_t node, phase, next;
	float w, tq;
	Rigid rm;
};
enum : uint32_t { CF_BLEND_FROM_DONE, CF_BLEND_TO_DONE, CF_ENTER_NEXT, CF_PLAYRATE, CF_IK };

struct CtlCtx {
	const CtlNode* nodes;
	const CtlOp* ops;
	const uint32_t* exprs; // {first op, ops} per expression
	const uint32_t* aux;
	const uint32_t* slots;   // RuntimeContext::animations: lmx_anim_add ids, LMX_ANIM_NONE for an empty slot
	const CtlClip* clips;
	const float* rm_t;       // 3 floats per entry
	const float* rm_r;       // 4 floats per entry
	const uint32_t* inputs;  // RuntimeContext::inputs, 4 words each: type, union
	const uint32_t* ik_leaf; // per IK ordinal: the leaf's bone index in the Animator's model, LMX_BONE_NONE
	const uint32_t* in;      // RuntimeContext::input_runtime: word k at in[k * stride]
	uint32_t* out;           // RuntimeContext::data
	uint32_t stride, rd, wr;
	uint32_t time_delta;
	float weight;
	Rigid root_motion;
	LmxBlendInstr* instrs;   // RuntimeContext::blendstack, decoded
	uint32_t n_instrs;
};

LMX_HD float ctl_f(uint32_t u) { return __builtin_bit_cast(float, u); }
LMX_HD uint32_t ctl_u(float f) { return __builtin_bit_cast(uint32_t, f); }
// The conversion to u32, on the number's bits (integer instructions only, the same on host and device): truncate, keep the low 32 bits of
// the 64-bit two's complement; 0 below 1, for NaN and from +-2^63 on.
LMX_HD uint32_t ctl_u32(float x) {
	const uint32_t u = __builtin_bit_cast(uint32_t, x);
	const int32_t e = (int32_t)((u >> 23) & 0xffu) - 127;
	if (e < 0 || e >= 63) return 0u;
	const uint32_t m = (u & 0x7fffffu) | 0x800000u; // |x| = m * 2^(e - 23)
	const uint32_t low = e >= 23 ? (e - 23 >= 32 ? 0u : m << (e - 23)) : m >> (23 - e);
	return (u >> 31) ? 0u - low : low;
}
LMX_HD uint32_t ctl_u32(double x) {
	const uint64_t u = __builtin_bit_cast(uint64_t, x);
	const int32_t e = (int32_t)((u >> 52) & 0x7ffu) - 1023;
	if (e < 0 || e >= 63) return 0u;
	const uint64_t m = (u & 0xfffffffffffffull) | 0x10000000000000ull; // |x| = m * 2^(e - 52)
	const uint32_t low = (uint32_t)(e >= 52 ? m << (e - 52) : m >> (52 - e));
	return (u >> 63) ? 0u - low : low;
}
LMX_HD int32_t ctl_i32(float x) { return (x >= -2147483648.f && x < 2147483648.f) ? (int32_t)x : (int32_t)0x80000000u; }
// fmodf(x, 1): x - trunc(x) is exact (the fraction of an fp32 number is one), the result carries x's sign (a zero too); inf and NaN give NaN
LMX_HD float ctl_fmod1(float x) { return __builtin_copysignf(x - __builtin_truncf(x), x); }

// Time (animation/animation.h:17-42, 180-183)
LMX_HD float time_seconds(uint32_t v) { return (float)((double)v / (double)LMX_TIME_ONE_SECOND); }
LMX_HD uint32_t time_from_seconds(float s) { return ctl_u32(s * (float)LMX_TIME_ONE_SECOND); }
LMX_HD uint32_t time_mul(uint32_t v, float t) { return ctl_u32((float)v * t); }
LMX_HD float time_div(uint32_t a, uint32_t b) { return (float)((double)a / (double)b); }
LMX_HD uint32_t time_lerp(uint32_t a, uint32_t b, float t) { return ctl_u32((double)a * (double)(1 - t) + (double)b * (double)t); }

LMX_HD uint32_t ctl_read(CtlCtx& c) { return c.in[(c.rd++) * c.stride]; }
LMX_HD void ctl_write(CtlCtx& c, uint32_t v) { c.out[(c.wr++) * c.stride] = v; }

// ValueNode::eval of a whole tree: the Value's first word
LMX_HD uint32_t ctl_eval(const CtlCtx& c, uint32_t expr) {
	const uint32_t first = c.exprs[2 * expr], n = c.exprs[2 * expr + 1];
	uint32_t st[LMX_CONTROLLER_MAX_VALUE_DEPTH];
	uint32_t sp = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const CtlOp op = c.ops[first + i];
		if (op.op == CN_INPUT) { st[sp++] = c.inputs[4 * op.a + 1]; continue; }
		if (op.op == CN_CONSTANT) { st[sp++] = op.a; continue; }
		const uint32_t u1 = st[--sp], u0 = st[--sp];
		const float v0 = ctl_f(u0), v1 = ctl_f(u1);
		uint32_t r = 0;
		switch (op.op) { // MathNode::eval, nodes.h:106-128
			case CN_CMP_GT: r = v0 > v1; break;
			case CN_CMP_GTE: r = v0 >= v1; break;
			case CN_CMP_LT: r = v0 < v1; break;
			case CN_CMP_LTE: r = v0 <= v1; break;
			case CN_CMP_NEQ: r = v0 != v1; break;
			case CN_CMP_EQ: r = v0 == v1; break;
			case CN_AND: r = u0 && u1; break;
			case CN_OR: r = u0 || u1; break;
			case CN_MUL: r = ctl_u(v0 * v1); break;
			case CN_DIV: r = ctl_u(v0 / v1); break;
			case CN_ADD: r = ctl_u(v0 + v1); break;
			default: r = ctl_u(v0 - v1); break; // CN_SUB
		}
		st[sp++] = r;
	}
	return st[0];
}
LMX_HD V3 ctl_eval_vec3(const CtlCtx& c, uint32_t expr) { // an INPUT or a CONSTANT of type VEC3
	const CtlOp op = c.ops[c.exprs[2 * expr]];
	if (op.op == CN_INPUT) return V3{ctl_f(c.inputs[4 * op.a + 1]), ctl_f(c.inputs[4 * op.a + 2]), ctl_f(c.inputs[4 * op.a + 3])};
	return V3{ctl_f(op.a), ctl_f(op.b), ctl_f(op.c)};
}
LMX_HD int32_t ctl_child_index(const CtlCtx& c, uint32_t expr, uint32_t n_children) { // toI32 and the clamp, nodes.cpp:164-165
	const int32_t i = ctl_i32(ctl_f(ctl_eval(c, expr)) + 0.5f);
	const int32_t lo = i > 0 ? i : 0, hi = (int32_t)n_children - 1;
	return lo < hi ? lo : hi;
}

// Animation::getRootMotion, animation.cpp:272-291
LMX_HD Rigid clip_root_motion(const CtlCtx& c, const CtlClip& a, uint32_t time) {
	Rigid tr = Rigid{V3{0, 0, 0}, Q4{0, 0, 0, 1}};
	const float frame = (float)((double)time / (double)LMX_TIME_ONE_SECOND * (double)a.fps);
	const uint32_t idx = ctl_u32(frame);
	if (idx < a.frame_count) {
		const float frame_t = frame - (float)idx;
		if (a.rm_r != LMX_ANIM_NONE) {
			const float* r = c.rm_r + 4 * (size_t)(a.rm_r + idx);
			tr.rot = nlerp(Q4{r[0], r[1], r[2], r[3]}, Q4{r[4], r[5], r[6], r[7]}, frame_t);
		}
		if (a.rm_t != LMX_ANIM_NONE) {
			const float* t = c.rm_t + 3 * (size_t)(a.rm_t + idx);
			tr.pos = lerp(V3{t[0], t[1], t[2]}, V3{t[3], t[4], t[5]}, frame_t);
		}
		return tr;
	}
	if (a.rm_r != LMX_ANIM_NONE) {
		const float* r = c.rm_r + 4 * (size_t)(a.rm_r + a.frame_count);
		tr.rot = Q4{r[0], r[1], r[2], r[3]};
	}
	if (a.rm_t != LMX_ANIM_NONE) {
		const float* t = c.rm_t + 3 * (size_t)(a.rm_t + a.frame_count);
		tr.pos = V3{t[0], t[1], t[2]};
	}
	return tr;
}
LMX_HD Rigid clip_root_motion_ex(const CtlCtx& c, const CtlClip& a, uint32_t t0, uint32_t t1) { // nodes.cpp:21-26
	return rigid_mul(rigid_inverted(clip_root_motion(c, a, t0)), clip_root_motion(c, a, t1));
}
LMX_HD Rigid clip_root_motion_between(const CtlCtx& c, const CtlClip& a, uint32_t t0_abs, uint32_t t1_abs) { // nodes.cpp:28-38
	const uint32_t t0 = t0_abs % a.length, t1 = t1_abs % a.length;
	if (t0 <= t1) return clip_root_motion_ex(c, a, t0, t1);
	const Rigid tr_0 = clip_root_motion_ex(c, a, t0, a.length);
	const Rigid tr_1 = clip_root_motion_ex(c, a, 0, t1);
	return rigid_mul(tr_0, tr_1);
}
LMX_HD Rigid rigid_interpolate(const Rigid& a, const Rigid& b, float t) { return Rigid{lerp(a.pos, b.pos, t), nlerp(a.rot, b.rot, t)}; } // math.cpp:863-868

LMX_HD void ctl_emit_sample(CtlCtx& c, uint32_t animation, float weight, uint32_t time, bool looped) {
	LmxBlendInstr ins = {};
	ins.op = LMX_BLEND_SAMPLE;
	ins.animation = animation;
	ins.weight = weight;
	ins.time = time;
	ins.looped = looped;
	ins.leaf_bone = LMX_BONE_NONE; // (the record lmx_anim_decode_blend_stack writes for a SAMPLE, field for field)
	c.instrs[c.n_instrs++] = ins;
}

// PoseNode::enter: every node's enter ends in at most one child's
LMX_HD void ctl_enter(CtlCtx& c, uint32_t node) {
	for (;;) {
		const CtlNode n = c.nodes[node];
		switch (n.type) {
			case CN_SELECT: { // nodes.cpp:209-219
				const uint32_t child = (uint32_t)ctl_child_index(c, n.w[3], n.w[2]);
				ctl_write(c, child);
				ctl_write(c, child);
				ctl_write(c, 0);
				node = c.aux[n.w[1] + child];
				break;
			}
			case CN_SWITCH: { // :310-318
				const uint32_t cond = ctl_eval(c, n.w[3]) != 0;
				ctl_write(c, cond);
				ctl_write(c, 0);
				node = cond ? n.w[1] : n.w[2];
				break;
			}
			case CN_PLAYRATE: node = n.w[1]; break;
			case CN_IK: node = n.w[4]; break;
			default: ctl_write(c, 0); return; // ANIMATION: Time(0); BLEND1D / BLEND2D: 0.f
		}
	}
}

// PoseNode::skip of a subtree of the input stream
LMX_HD void ctl_skip(CtlCtx& c, uint32_t node) {
	uint32_t pending[LMX_CONTROLLER_MAX_POSE_DEPTH + 1];
	uint32_t sp = 0;
	pending[sp++] = node;
	while (sp) {
		const CtlNode n = c.nodes[pending[--sp]];
		switch (n.type) {
			case CN_SELECT: { // :221-227
				const uint32_t from = ctl_read(c), to = ctl_read(c);
				(void)ctl_read(c);
				if (from != to) pending[sp++] = c.aux[n.w[1] + to];
				pending[sp++] = c.aux[n.w[1] + from];
				break;
			}
			case CN_SWITCH: { // :320-326
				const uint32_t d = ctl_read(c);
				(void)ctl_read(c);
				const bool current = (d & 0xffu) != 0, switching = (d & 0xff00u) != 0;
				pending[sp++] = current ? n.w[1] : n.w[2];
				if (switching) pending[sp++] = current ? n.w[2] : n.w[1];
				break;
			}
			case CN_PLAYRATE: pending[sp++] = n.w[1]; break;
			case CN_IK: pending[sp++] = n.w[4]; break;
			default: (void)ctl_read(c); break;
		}
	}
}

LMX_HD void ctl_update_animation(CtlCtx& c, const CtlNode& n) { // nodes.cpp:92-117
	uint32_t t = ctl_read(c);
	uint32_t prev_t = t;
	t += c.time_delta;
	const uint32_t id = c.slots[n.w[0]];
	const bool looped = (n.w[1] & CTL_ANIMATION_LOOPED) != 0;
	if (id != LMX_ANIM_NONE) {
		const CtlClip a = c.clips[id];
		if (!looped) {
			t = t < a.length ? t : a.length;
			prev_t = prev_t < a.length ? prev_t : a.length;
		}
		c.root_motion = clip_root_motion_between(c, a, prev_t, t);
	} else c.root_motion = Rigid{V3{0, 0, 0}, Q4{0, 0, 0, 1}};
	ctl_write(c, t);
	ctl_emit_sample(c, id, c.weight, t, looped);
}

LMX_HD void ctl_update_blend1d(CtlCtx& c, const CtlNode& n) { // nodes.cpp:607-623, 644-688
	float relt = ctl_f(ctl_read(c));
	const float relt0 = relt;
	const float input_val = ctl_f(ctl_eval(c, n.w[2]));
	const uint32_t* ch = c.aux + n.w[0];
	const uint32_t count = n.w[1];
	uint32_t ia = 0, ib = 0xffffffffu;
	float pt = 0;
	if (input_val > ctl_f(ch[0])) {
		if (input_val >= ctl_f(ch[2 * (count - 1)])) ia = count - 1;
		else {
			for (uint32_t i = 1; i < count; ++i) {
				if (input_val < ctl_f(ch[2 * i])) {
					pt = (input_val - ctl_f(ch[2 * (i - 1)])) / (ctl_f(ch[2 * i]) - ctl_f(ch[2 * (i - 1)]));
					ia = i - 1;
					ib = i;
					break;
				}
			}
		}
	}
	const bool has_b = ib != 0xffffffffu;
	const uint32_t id_a = c.slots[ch[2 * ia + 1]];
	const CtlClip a = c.clips[id_a];
	CtlClip b = a;
	if (has_b) b = c.clips[c.slots[ch[2 * ib + 1]]];
	const uint32_t wlen = time_lerp(a.length, b.length, pt);
	relt = relt + time_div(c.time_delta, wlen);
	relt = ctl_fmod1(relt);
	c.root_motion = clip_root_motion_between(c, a, time_mul(a.length, relt0), time_mul(a.length, relt));
	if (has_b) {
		const Rigid tr1 = clip_root_motion_between(c, b, time_mul(b.length, relt0), time_mul(b.length, relt));
		c.root_motion = rigid_interpolate(c.root_motion, tr1, pt);
	}
	ctl_write(c, ctl_u(relt));
	ctl_emit_sample(c, id_a, c.weight, time_mul(a.length, relt), true);
	if (has_b) ctl_emit_sample(c, id_a, c.weight * pt, time_mul(b.length, relt), true); // pair.a->slot with anim_b's length, :681-687
}

LMX_HD bool ctl_barycentric(float px, float py, float ax, float ay, float bx, float by, float cx, float cy, float& u, float& v) { // nodes.cpp:435-448
	const float abx = bx - ax, aby = by - ay, acx = cx - ax, acy = cy - ay, apx = px - ax, apy = py - ay;
	const float d00 = abx * abx + aby * aby;
	const float d01 = abx * acx + aby * acy;
	const float d11 = acx * acx + acy * acy;
	const float d20 = apx * abx + apy * aby;
	const float d21 = apx * acx + apy * acy;
	const float denom = d00 * d11 - d01 * d01;
	u = (d11 * d20 - d01 * d21) / denom;
	v = (d00 * d21 - d01 * d20) / denom;
	return u >= 0.f && v >= 0.f && u + v <= 1.f;
}

LMX_HD void ctl_update_blend2d(CtlCtx& c, const CtlNode& n) { // nodes.cpp:450-473, 504-568
	float relt = ctl_f(ctl_read(c));
	const float relt0 = relt;
	const float x = ctl_f(ctl_eval(c, n.w[4])), y = ctl_f(ctl_eval(c, n.w[5]));
	const uint32_t* ch = c.aux + n.w[0];
	const uint32_t* tri = c.aux + n.w[2];
	uint32_t sa = ch[2], sb = ch[2], sc = ch[2];
	float ta = 1, tb = 0, tc = 0;
	for (uint32_t i = 0; i < n.w[3]; ++i) {
		const uint32_t* ca = ch + 3 * tri[3 * i], *cb = ch + 3 * tri[3 * i + 1], *cc = ch + 3 * tri[3 * i + 2];
		float u, v;
		if (!ctl_barycentric(x, y, ctl_f(ca[0]), ctl_f(ca[1]), ctl_f(cb[0]), ctl_f(cb[1]), ctl_f(cc[0]), ctl_f(cc[1]), u, v)) continue;
		sa = ca[2]; sb = cb[2]; sc = cc[2];
		ta = 1 - u - v; tb = u; tc = v;
		break;
	}
	const uint32_t id_a = c.slots[sa], id_b = c.slots[sb], id_c = c.slots[sc];
	if (id_a == LMX_ANIM_NONE || id_b == LMX_ANIM_NONE || id_c == LMX_ANIM_NONE) { // :515-518: root_motion keeps last frame's value
		ctl_write(c, ctl_u(relt));
		return;
	}
	const CtlClip a = c.clips[id_a], b = c.clips[id_b], cl = c.clips[id_c];
	const uint32_t wlen = time_mul(a.length, ta) + time_mul(b.length, tb) + time_mul(cl.length, tc);
	relt = relt + time_div(c.time_delta, wlen);
	relt = ctl_fmod1(relt);
	c.root_motion = clip_root_motion_between(c, a, time_mul(a.length, relt0), time_mul(a.length, relt));
	if (tb > 0) {
		const Rigid tr1 = clip_root_motion_between(c, b, time_mul(b.length, relt0), time_mul(b.length, relt));
		c.root_motion = rigid_interpolate(c.root_motion, tr1, tb / (ta + tb));
	}
	if (tc > 0) {
		const Rigid tr1 = clip_root_motion_between(c, cl, time_mul(cl.length, relt0), time_mul(cl.length, relt));
		c.root_motion = rigid_interpolate(c.root_motion, tr1, tc);
	}
	ctl_write(c, ctl_u(relt));
	ctl_emit_sample(c, id_a, c.weight, time_mul(a.length, relt), true);
	if (tb > 0) ctl_emit_sample(c, id_b, c.weight * (tb / (ta + tb)), time_mul(b.length, relt), true);
	if (tc > 0) ctl_emit_sample(c, id_c, c.weight * (tc / (ta + tb + tc)), time_mul(cl.length, relt), true);
}

// Controller::update's m_root->update(ctx). `stack`: LMX_CONTROLLER_MAX_POSE_DEPTH frames.
LMX_HD void ctl_update(CtlCtx& c, uint32_t root, CtlFrame* stack) {
	uint32_t sp = 0, cur = root;
	bool descend = true;
	for (;;) {
		if (descend) {
			const CtlNode n = c.nodes[cur];
			switch (n.type) {
				case CN_ANIMATION: ctl_update_animation(c, n); descend = false; break;
				case CN_BLEND1D: ctl_update_blend1d(c, n); descend = false; break;
				case CN_BLEND2D: ctl_update_blend2d(c, n); descend = false; break;
				case CN_SELECT:   // nodes.cpp:161-207
				case CN_SWITCH: { // :262-308, the same machine: from / to are the running and the entered child
					uint32_t from, to, t, blend_length = n.w[0], word0 = 0, word1 = 0;
					uint32_t from_node, to_node;
					bool blending, start;
					if (n.type == CN_SELECT) {
						from = ctl_read(c); to = ctl_read(c); t = ctl_read(c);
						const uint32_t child = (uint32_t)ctl_child_index(c, n.w[3], n.w[2]);
						blending = from != to;
						start = !blending && child != from;
						if (start) to = child;
						from_node = c.aux[n.w[1] + from];
						to_node = c.aux[n.w[1] + to];
					} else {
						const uint32_t d = ctl_read(c);
						t = ctl_read(c);
						bool current = (d & 0xffu) != 0;
						blending = (d & 0xff00u) != 0;
						const bool condition = ctl_eval(c, n.w[3]) != 0;
						start = !blending && current != condition;
						if (start) current = condition;
						from = 0; to = current; // `to`: RuntimeData::current
						to_node = current ? n.w[1] : n.w[2];
						from_node = (blending || start) ? (current ? n.w[2] : n.w[1]) : to_node;
					}
					bool finished = false;
					if (blending) {
						t += c.time_delta;
						finished = t > blend_length;
						if (finished) t = 0;
					} else if (start) t = 0;
					else t += c.time_delta;
					if (n.type == CN_SELECT) {
						word0 = finished ? to : from;
						word1 = to;
					} else word0 = to | ((blending && !finished) || start ? 0x100u : 0u);
					if (finished) ctl_skip(c, from_node); // "TODO root motion in data.from": the running child is dropped unread
					ctl_write(c, word0);
					if (n.type == CN_SELECT) ctl_write(c, word1);
					ctl_write(c, t);
					if (finished) cur = to_node;
					else if (blending) {
						CtlFrame& f = stack[sp++];
						f.node = cur; f.phase = CF_BLEND_FROM_DONE; f.next = to_node;
						f.tq = time_seconds(t) / time_seconds(blend_length);
						cur = from_node;
					} else if (start) {
						CtlFrame& f = stack[sp++];
						f.node = cur; f.phase = CF_ENTER_NEXT; f.next = to_node;
						cur = from_node;
					} else cur = from_node;
					break;
				}
				case CN_PLAYRATE: { // :736-741
					CtlFrame& f = stack[sp++];
					f.node = cur; f.phase = CF_PLAYRATE;
					f.tq = time_seconds(c.time_delta);
					const float v = ctl_f(ctl_eval(c, n.w[0]));
					c.time_delta = time_mul(c.time_delta, 0.f > v ? 0.f : v);
					cur = n.w[1];
					break;
				}
				default: { // CN_IK, :357-369
					CtlFrame& f = stack[sp++];
					f.node = cur; f.phase = CF_IK;
					cur = n.w[4];
					break;
				}
			}
			continue;
		}
		if (!sp) return;
		CtlFrame& f = stack[sp - 1];
		switch (f.phase) {
			case CF_BLEND_FROM_DONE: {
				const float lo = f.tq > 0.f ? f.tq : 0.f; // clamp(t, 0.f, 1.f) = minimum(maximum(t, 0), 1): NaN becomes 0
				const float t = lo < 1.f ? lo : 1.f;
				f.w = c.weight;
				c.weight *= t;
				f.rm = c.root_motion;
				f.phase = CF_BLEND_TO_DONE;
				cur = f.next;
				descend = true;
				break;
			}
			case CF_BLEND_TO_DONE:
				c.weight = f.w;
				c.root_motion = rigid_interpolate(f.rm, c.root_motion, f.tq);
				--sp;
				break;
			case CF_ENTER_NEXT:
				ctl_enter(c, f.next);
				--sp;
				break;
			case CF_PLAYRATE:
				c.time_delta = time_from_seconds(f.tq);
				--sp;
				break;
			default: { // CF_IK
				const CtlNode n = c.nodes[f.node];
				float alpha = ctl_f(ctl_eval(c, n.w[2]));
				if (alpha > 0) {
					alpha = 1.f < alpha ? 1.f : alpha;
					const V3 p = ctl_eval_vec3(c, n.w[3]);
					LmxBlendInstr ins = {};
					ins.op = LMX_BLEND_IK;
					ins.alpha = alpha; // x RuntimeContext::weight, which is 1 when evalBlendStack runs (only the nodes write it, and they restore it)
					ins.target[0] = p.x; ins.target[1] = p.y; ins.target[2] = p.z;
					ins.leaf_bone = c.ik_leaf[n.w[1]];
					ins.bones_count = n.w[0];
					c.instrs[c.n_instrs++] = ins;
				}
				--sp;
				break;
			}
		}
	}
}

// ---- the host side (lmx_controller_program.cpp) ----
struct ControllerProgram {
	std::vector<CtlNode> nodes;
	std::vector<CtlOp> ops;
	std::vector<uint32_t> exprs, aux;
	std::vector<uint32_t> input_types;   // Controller::Input::type
	std::vector<uint8_t> slot_required;  // per slot: an ANIMATION or BLEND1D node names it (an empty slot there is a null dereference in the reference)
	std::vector<uint64_t> ik_leaf_hash;  // per IK node: IKNode::m_leaf_bone
	std::vector<uint32_t> ik_bones;      // ... and m_bones_count
	std::vector<uint32_t> enter_image;   // RuntimeContext::data after Controller::createRuntime: inputs are zero there, so it depends on the program alone
	uint32_t root = 0, version = 0, n_slots = 0, n_entries = 0;
	uint32_t state_words = 0, max_instrs = 0, pose_depth = 0, value_depth = 0;
};
// Decodes and validates a compiled controller resource (Controller::deserialize, controller.cpp:104-140). Reads nothing outside
// [bytes, bytes + n_bytes). false: `error` says why, `out` is unspecified.
bool controller_program_parse(const uint8_t* bytes, uint64_t n_bytes, ControllerProgram& out, std::string& error);

} // namespace lmx
