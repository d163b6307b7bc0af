// lmx_controller_program.cpp — decoder and validator of a compiled animation controller (Controller::deserialize, controller.cpp:104-140,
// and the nodes' deserialize methods, animation/nodes.cpp). Plain C++, no device: also built on its own by tests/cpp/controller_fuzz.cpp.
// Everything the VM of lmx_controller_program.h indexes with is checked here, once; the VM carries no checks.
#include "lmx_controller_program.h"
#include "lumix_mi355.h"

#include <cstdio>
#include <cstring>

namespace lmx {

namespace {

constexpr uint32_t CONTROLLER_MAGIC = 0x5f4c4143u; // '_LAC', controller.cpp:85
constexpr uint32_t VERSION_BONE_NAME_HASH = 1, VERSION_LATEST = 2; // ControllerVersion, controller.h:64-69

struct Parser {
	const uint8_t* bytes;
	uint64_t size, pos = 0;
	ControllerProgram& p;
	std::string& error;

	bool fail(const char* what) {
		char buf[160];
		snprintf(buf, sizeof(buf), "%s (at byte %llu of %llu)", what, (unsigned long long)pos, (unsigned long long)size);
		error = buf;
		return false;
	}
	bool read(void* dst, uint64_t n) {
		if (n > size - pos) return fail("the stream is truncated");
		if (n) memcpy(dst, bytes + pos, n);
		pos += n;
		return true;
	}
	bool u32(uint32_t& v) { return read(&v, 4); }
	bool count(uint32_t& n, uint64_t item_size) { // readArray's i32 size (stream.h:140-144) and the bytes it promises
		int32_t s;
		if (!read(&s, 4)) return false;
		if (s < 0) return fail("negative array size");
		if ((uint64_t)s * item_size > size - pos) return fail("the stream is truncated");
		n = (uint32_t)s;
		return true;
	}

	static bool is_pose(uint32_t t) { return t == CN_ANIMATION || t == CN_BLEND1D || t == CN_BLEND2D || t == CN_SELECT || t == CN_SWITCH || t == CN_PLAYRATE || t == CN_IK; }
	static bool is_math(uint32_t t) { return (t >= CN_CMP_EQ && t <= CN_SUB) || t == CN_AND || t == CN_OR; }

	// One value node and its subtree, appended in postfix order. `type`: the static Value::Type of its result; `need`: the operands the
	// evaluation holds at once.
	bool value(uint32_t depth, uint32_t& type, uint32_t& need) {
		uint32_t t;
		if (!u32(t)) return false;
		if (depth > LMX_CONTROLLER_MAX_VALUE_DEPTH) return fail("value tree nested deeper than LMX_CONTROLLER_MAX_VALUE_DEPTH");
		if (t == CN_INPUT) {
			uint32_t idx;
			if (!u32(idx)) return false;
			if (idx >= p.input_types.size()) return fail("INPUT index outside m_inputs");
			p.ops.push_back(CtlOp{CN_INPUT, idx, 0, 0});
			type = p.input_types[idx];
			need = 1;
			return true;
		}
		if (t == CN_CONSTANT) {
			uint32_t v[4];
			if (!read(v, 16)) return false;
			if (v[0] > LMX_VALUE_VEC3) return fail("CONSTANT of unknown type");
			if (v[0] == LMX_VALUE_BOOL) v[1] = (v[1] & 0xffu) != 0; // Value::b is the union's first byte
			p.ops.push_back(CtlOp{CN_CONSTANT, v[1], v[2], v[3]});
			type = v[0];
			need = 1;
			return true;
		}
		if (!is_math(t)) return fail(t < CN_TYPE_COUNT ? "a pose node where a value node belongs" : "unknown node type");
		uint32_t t0, t1, n0, n1;
		if (!value(depth + 1, t0, n0) || !value(depth + 1, t1, n1)) return false;
		if (t == CN_AND || t == CN_OR) {
			if (t0 != LMX_VALUE_BOOL || t1 != LMX_VALUE_BOOL) return fail("AND / OR reads .b of a value that is not a BOOL");
			type = LMX_VALUE_BOOL;
		} else {
			if (t0 == LMX_VALUE_BOOL || t1 == LMX_VALUE_BOOL) return fail("a math node reads .f of a BOOL");
			type = t >= CN_MUL ? LMX_VALUE_NUMBER : LMX_VALUE_BOOL;
		}
		p.ops.push_back(CtlOp{t, 0, 0, 0});
		need = n0 > n1 + 1 ? n0 : n1 + 1;
		return true;
	}
	// A whole value tree as an expression; its result must be `want` (the toFloat / toI32 / toBool / toVec3 assert, controller.h:33-36)
	bool expr(uint32_t want, uint32_t& out) {
		const uint32_t first = (uint32_t)p.ops.size();
		uint32_t type, need;
		if (!value(1, type, need)) return false;
		if (type != want) return fail("a value tree's type breaks the assert of toFloat / toI32 / toBool / toVec3");
		if (need > LMX_CONTROLLER_MAX_VALUE_DEPTH) return fail("value tree needs more operands than LMX_CONTROLLER_MAX_VALUE_DEPTH");
		if (need > p.value_depth) p.value_depth = need;
		out = (uint32_t)(p.exprs.size() / 2);
		p.exprs.push_back(first);
		p.exprs.push_back((uint32_t)p.ops.size() - first);
		return true;
	}

	// One pose node and its subtree. words / instrs: the upper bounds of what an update writes of runtime data and emits.
	bool pose(uint32_t t, uint32_t depth, uint32_t& out, uint32_t& words, uint32_t& instrs) {
		if (!is_pose(t)) return fail(t == CN_LAYERS || t == CN_TREE || t == CN_OUTPUT || t == CN_NONE ? "LAYERS / TREE / OUTPUT / NONE: Node::create has no runtime node for it"
			: t < CN_TYPE_COUNT ? "a value node where a pose node belongs" : "unknown node type");
		if (depth > LMX_CONTROLLER_MAX_POSE_DEPTH) return fail("pose nodes nested deeper than LMX_CONTROLLER_MAX_POSE_DEPTH");
		if (depth > p.pose_depth) p.pose_depth = depth;
		out = (uint32_t)p.nodes.size();
		p.nodes.push_back(CtlNode{});
		CtlNode n = {};
		n.type = t;
		auto child = [&](uint32_t& node, uint32_t& w, uint32_t& i) {
			uint32_t ct;
			return u32(ct) && pose(ct, depth + 1, node, w, i);
		};
		switch (t) {
			case CN_ANIMATION: {
				if (!u32(n.w[0]) || !u32(n.w[1])) return false;
				if (n.w[0] >= p.n_slots) return fail("ANIMATION slot outside m_animation_slots_count");
				p.slot_required[n.w[0]] = 1;
				words = 1;
				instrs = 1;
				break;
			}
			case CN_BLEND1D: {
				uint32_t cnt;
				if (!count(cnt, 8)) return false;
				if (!cnt) return fail("BLEND1D without children");
				n.w[0] = (uint32_t)p.aux.size();
				n.w[1] = cnt;
				for (uint32_t i = 0; i < cnt; ++i) {
					uint32_t c[2];
					if (!read(c, 8)) return false;
					if (c[1] >= p.n_slots) return fail("BLEND1D slot outside m_animation_slots_count");
					p.slot_required[c[1]] = 1;
					p.aux.push_back(c[0]);
					p.aux.push_back(c[1]);
				}
				if (!expr(LMX_VALUE_NUMBER, n.w[2])) return false;
				words = 1;
				instrs = 2;
				break;
			}
			case CN_BLEND2D: {
				uint32_t cnt, tris;
				if (!count(cnt, 12)) return false;
				if (!cnt) return fail("BLEND2D without children");
				n.w[0] = (uint32_t)p.aux.size();
				n.w[1] = cnt;
				for (uint32_t i = 0; i < cnt; ++i) {
					uint32_t c[3];
					if (!read(c, 12)) return false;
					if (c[2] >= p.n_slots) return fail("BLEND2D slot outside m_animation_slots_count");
					p.aux.insert(p.aux.end(), c, c + 3);
				}
				if (!count(tris, 20)) return false;
				n.w[2] = (uint32_t)p.aux.size();
				n.w[3] = tris;
				for (uint32_t i = 0; i < tris; ++i) {
					uint32_t c[5]; // a, b, c, circumcircle_center
					if (!read(c, 20)) return false;
					if (c[0] >= cnt || c[1] >= cnt || c[2] >= cnt) return fail("BLEND2D triangle index outside the children");
					p.aux.insert(p.aux.end(), c, c + 3);
				}
				if (!expr(LMX_VALUE_NUMBER, n.w[4]) || !expr(LMX_VALUE_NUMBER, n.w[5])) return false;
				words = 1;
				instrs = 3;
				break;
			}
			case CN_SELECT: {
				uint32_t cnt;
				if (!u32(n.w[0]) || !u32(cnt)) return false;
				if (!cnt) return fail("SELECT without children");
				if ((uint64_t)cnt * 8 > size - pos) return fail("the stream is truncated"); // a child is at least a type and a word
				std::vector<uint32_t> kids(cnt);
				uint32_t w1 = 0, w2 = 0, i1 = 0, i2 = 0; // the two largest children
				for (uint32_t i = 0; i < cnt; ++i) {
					uint32_t w, k;
					if (!child(kids[i], w, k)) return false;
					if (w > w1) { w2 = w1; w1 = w; } else if (w > w2) w2 = w;
					if (k > i1) { i2 = i1; i1 = k; } else if (k > i2) i2 = k;
				}
				n.w[1] = (uint32_t)p.aux.size();
				n.w[2] = cnt;
				p.aux.insert(p.aux.end(), kids.begin(), kids.end());
				if (!expr(LMX_VALUE_NUMBER, n.w[3])) return false;
				words = 3 + w1 + w2;
				instrs = i1 + i2;
				break;
			}
			case CN_SWITCH: {
				uint32_t wt, wf, it, ifl;
				if (!u32(n.w[0]) || !child(n.w[1], wt, it) || !child(n.w[2], wf, ifl) || !expr(LMX_VALUE_BOOL, n.w[3])) return false;
				words = 2 + wt + wf;
				instrs = it + ifl;
				break;
			}
			case CN_PLAYRATE: {
				if (!expr(LMX_VALUE_NUMBER, n.w[0]) || !child(n.w[1], words, instrs)) return false;
				break;
			}
			default: { // CN_IK
				uint64_t leaf = 0; // the outdated form leaves m_leaf_bone default-constructed
				if (!u32(n.w[0])) return false;
				if (p.version <= VERSION_BONE_NAME_HASH) {
					uint32_t skipped;
					if (!u32(skipped)) return false;
				} else if (!read(&leaf, 8)) return false;
				if (!n.w[0] || n.w[0] > LMX_IK_MAX_BONES) return fail("IK bones_count is 0 or above LMX_IK_MAX_BONES");
				n.w[1] = (uint32_t)p.ik_leaf_hash.size();
				p.ik_leaf_hash.push_back(leaf);
				p.ik_bones.push_back(n.w[0]);
				if (!expr(LMX_VALUE_NUMBER, n.w[2]) || !expr(LMX_VALUE_VEC3, n.w[3]) || !child(n.w[4], words, instrs)) return false;
				instrs += 1;
				break;
			}
		}
		p.nodes[out] = n;
		return true;
	}

	bool run() {
		uint32_t magic, n_inputs;
		if (!u32(magic) || !u32(p.version)) return false;
		if (magic != CONTROLLER_MAGIC) return fail("not an animation controller (magic)");
		if (p.version > VERSION_LATEST) return fail("unsupported ControllerVersion");
		if (!count(n_inputs, 36)) return false; // Controller::Input: a type and a StaticString<32>
		for (uint32_t i = 0; i < n_inputs; ++i) {
			uint32_t rec[9];
			if (!read(rec, 36)) return false;
			if (rec[0] > LMX_VALUE_VEC3) return fail("input of unknown type");
			p.input_types.push_back(rec[0]);
		}
		if (!u32(p.n_slots) || !u32(p.n_entries)) return false;
		if (p.n_slots > (1u << 20)) return fail("m_animation_slots_count above 2^20");
		p.slot_required.assign(p.n_slots, 0);
		for (uint32_t i = 0; i < p.n_entries; ++i) {
			uint32_t slot, set;
			if (!u32(slot) || !u32(set)) return false;
			if (slot >= p.n_slots) return fail("animation entry names a slot outside m_animation_slots_count");
			while (pos < size && bytes[pos]) ++pos; // readString, stream.cpp:424-436
			if (pos >= size) return fail("the stream is truncated");
			++pos;
		}
		uint32_t root_type, words = 0, instrs = 0;
		if (!u32(root_type) || !pose(root_type, 1, p.root, words, instrs)) return false;
		p.state_words = words;
		p.max_instrs = instrs;
		return true;
	}
};

} // namespace

bool controller_program_parse(const uint8_t* bytes, uint64_t n_bytes, ControllerProgram& out, std::string& error) {
	out = ControllerProgram();
	if (!bytes && n_bytes) {
		error = "null bytes";
		return false;
	}
	Parser ps{bytes, n_bytes, 0, out, error};
	if (!ps.run()) return false;
	// Controller::createRuntime, controller.cpp:51-67: m_root->enter with every input zero and typed
	std::vector<uint32_t> inputs(4 * out.input_types.size() + 4, 0u);
	for (size_t i = 0; i < out.input_types.size(); ++i) inputs[4 * i] = out.input_types[i];
	out.enter_image.assign(out.state_words, 0u);
	CtlCtx c = {};
	c.nodes = out.nodes.data();
	c.ops = out.ops.data();
	c.exprs = out.exprs.data();
	c.aux = out.aux.data();
	c.inputs = inputs.data();
	c.out = out.enter_image.data();
	c.stride = 1;
	ctl_enter(c, out.root);
	out.enter_image.resize(c.wr);
	return true;
}

} // namespace lmx

extern "C" int lmx_anim_controller_check(const void* bytes, uint64_t n_bytes, LmxControllerInfo* out_info, void* out_enter_image, uint32_t capacity_bytes, char* out_error,
	uint32_t error_capacity) {
	if (out_error && error_capacity) out_error[0] = 0;
	if (!bytes && n_bytes) return LMX_ERR_INVALID_ARGUMENT;
	lmx::ControllerProgram p;
	std::string error;
	if (!lmx::controller_program_parse((const uint8_t*)bytes, n_bytes, p, error)) {
		if (out_error && error_capacity) snprintf(out_error, error_capacity, "%s", error.c_str());
		return LMX_ERR_INVALID;
	}
	if (out_info) {
		LmxControllerInfo info = {};
		info.version = p.version;
		info.n_inputs = (uint32_t)p.input_types.size();
		info.n_slots = p.n_slots;
		info.n_entries = p.n_entries;
		info.n_nodes = (uint32_t)p.nodes.size();
		info.n_ik = (uint32_t)p.ik_bones.size();
		info.state_bytes = 4 * p.state_words;
		info.max_instrs = p.max_instrs;
		info.enter_bytes = 4 * (uint32_t)p.enter_image.size();
		info.pose_depth = p.pose_depth;
		info.value_depth = p.value_depth;
		*out_info = info;
	}
	if (out_enter_image) {
		if (capacity_bytes < 4 * p.enter_image.size()) return LMX_ERR_CAPACITY;
		if (!p.enter_image.empty()) memcpy(out_enter_image, p.enter_image.data(), 4 * p.enter_image.size());
	}
	return LMX_OK;
}
