// lmx_particle_program.cpp — decodes the byte stream of a particle emitter's programs into the fixed-width records of
// lmx_particle_program.h and refuses everything that could make a kernel leave a buffer. Plain C++: no HIP, no device.
//
// The layout is InputMemoryStream::read of the engine (no padding between items): a u8 InstructionType, then per instruction
// DataStream operands of 8 bytes {u8 type, u8 index, 2 pad, float value}, and for RAND two floats, GRADIENT a u32 count with count keys and
// count values, EMIT a u32 emitter, CMP a condition and a u16 block size, CMP_ELSE a condition and two u16 block sizes, MESH / SPLINE a
// destination, one operand and a trailing u8 (the subindex). The update program starts at byte 0, the emit program at emit_offset, the output program at output_offset.
#include "lmx_particle_program.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace lmx {

namespace {

enum Section { SEC_UPDATE, SEC_EMIT, SEC_OUTPUT };
enum Pos { POS_DST, POS_SRC, POS_SRC_STREAM /* getStream(): channel or register only */, POS_SRC_MOV_OUT, POS_SRC_MOV };

struct Decoder {
	const ParticleProgramDesc& d;
	ParticleProgram& out;
	std::string& error;
	Section section = SEC_UPDATE;
	bool in_emit_block = false;
	bool unsupported = false; // the refusal is of a well-formed MESH / SPLINE the device does not run (PD_UNSUPPORTED)
	uint32_t group = 0; // whole-chunk conditionals of the update program seen so far

	Decoder(const ParticleProgramDesc& desc, ParticleProgram& o, std::string& e) : d(desc), out(o), error(e) {}

	bool bad(uint32_t at, const char* what) {
		char buf[160];
		snprintf(buf, sizeof(buf), "particle program, byte %u: %s", at, what);
		error = buf;
		return false;
	}
	bool room(uint32_t pos, uint32_t n, uint32_t limit) const { return pos <= limit && n <= limit - pos; }
	template <typename T> T get(uint32_t pos) const {
		T v;
		memcpy(&v, d.bytes + pos, sizeof(T));
		return v;
	}

	uint32_t registers_here() const {
		const uint32_t n = d.registers_count + (section == SEC_EMIT ? d.emit_inputs_count : 0);
		return n < PARTICLE_MAX_REGISTERS ? n : PARTICLE_MAX_REGISTERS;
	}

	bool operand(uint32_t& pos, uint32_t limit, bool scalar, Pos where, ParticleOperand& o) {
		if (!room(pos, 8, limit)) return bad(pos, "operand runs past its block");
		o.type = d.bytes[pos];
		o.index = d.bytes[pos + 1];
		o.pad = 0;
		o.value = get<float>(pos + 4);
		const uint32_t at = pos;
		pos += 8;
		switch (o.type) {
			case PS_CHANNEL:
				if (o.index >= d.channels_count) return bad(at, "channel index out of range");
				return true;
			case PS_REGISTER:
				if (o.index >= registers_here()) return bad(at, "register index out of range");
				return true;
			case PS_OUT:
				if (in_emit_block) {
					if (o.index >= 16) return bad(at, "emit output index out of range");
				} else {
					if (section != SEC_OUTPUT) return bad(at, "output operand outside the output program");
					if (o.index >= d.outputs_count) return bad(at, "output index out of range");
				}
				if (where == POS_DST) return true;
				if (scalar && where == POS_SRC) return true;
				return bad(at, "output operand cannot be read here");
			case PS_LITERAL:
				if (where == POS_SRC || where == POS_SRC_MOV_OUT || where == POS_SRC_MOV) return true;
				return bad(at, where == POS_DST ? "a literal is no destination" : "operand must be a channel or a register");
			case PS_SYSTEM_VALUE:
				if (o.index >= PSV_COUNT) return bad(at, "system value index out of range");
				if (where == POS_SRC || where == POS_SRC_MOV) return true;
				return bad(at, where == POS_DST ? "a system value is no destination" : "a system value cannot be read here");
			case PS_GLOBAL:
				if (o.index >= d.n_globals) return bad(at, "global index out of range");
				if (where == POS_SRC || where == POS_SRC_MOV_OUT) return true;
				return bad(at, where == POS_DST ? "a global is no destination" : "a global cannot be read here");
			default: return bad(at, "stream type out of range");
		}
	}

	static int n_sources(uint8_t op) {
		switch (op) {
			case P_COS: case P_SIN: case P_NOISE: case P_SQRT: case P_MOV: case P_NOT: return 1;
			case P_ADD: case P_SUB: case P_MUL: case P_DIV: case P_MOD: case P_LT: case P_GT: case P_AND: case P_OR: case P_MAX: case P_MIN: return 2;
			case P_MULTIPLY_ADD: case P_MIX: case P_BLEND: return 3;
			default: return -1;
		}
	}

	// dst + sources of an arithmetic instruction
	bool arith(uint8_t op, uint32_t& pos, uint32_t limit, bool scalar, ParticleRec& r, uint16_t* wmask) {
		const int n = n_sources(op);
		if (!operand(pos, limit, scalar, POS_DST, r.o[0])) return false;
		if (r.o[0].type == PS_CHANNEL && wmask) *wmask |= (uint16_t)(1u << r.o[0].index);
		Pos where = POS_SRC;
		if (!scalar) {
			if (op == P_COS || op == P_SIN || op == P_NOISE || op == P_SQRT || op == P_MOD) where = POS_SRC_STREAM; // ProcessHelper::run1
			if (op == P_MOV) where = r.o[0].type == PS_OUT ? POS_SRC_MOV_OUT : POS_SRC_MOV;
		}
		for (int i = 0; i < n; ++i)
			if (!operand(pos, limit, scalar, where, r.o[1 + i])) return false;
		return true;
	}

	bool rand_op(uint32_t& pos, uint32_t limit, bool scalar, ParticleRec& r, uint16_t* wmask) {
		if (!operand(pos, limit, scalar, POS_DST, r.o[0])) return false;
		if (r.o[0].type == PS_CHANNEL && wmask) *wmask |= (uint16_t)(1u << r.o[0].index);
		if (!room(pos, 8, limit)) return bad(pos, "RAND runs past its block");
		r.o[1].value = get<float>(pos);
		r.o[2].value = get<float>(pos + 4);
		pos += 8;
		r.a = out.rand_count++;
		return true;
	}

	// MESH (run :741-774) and SPLINE (run :775-798, processChunk :1189-1219): dst, one operand, a u8 subindex. Without a declared source the
	// decoding stops here, as it always did, and the caller refuses the program.
	bool source_op(uint8_t op, uint32_t at, uint32_t& pos, uint32_t limit, bool scalar, ParticleRec& r, uint16_t* wmask) {
		const bool is_mesh = op == P_MESH;
		out.has_mesh_or_spline = true;
		(is_mesh ? out.has_mesh : out.has_spline) = true;
		if (!(d.sources & (is_mesh ? PARTICLE_SRC_MESH : PARTICLE_SRC_SPLINE))) {
			out.stopped = true;
			return true;
		}
		if (in_emit_block) return unsupported_form(at, "MESH / SPLINE inside an EMIT block: the reference's early return leaves the outer run in the middle of the block");
		if (is_mesh && !scalar) return unsupported_form(at, "MESH outside a conditional block or the emit program: the reference asserts");
		if (!operand(pos, limit, scalar, POS_DST, r.o[0])) return false;
		if (!operand(pos, limit, scalar, scalar ? POS_SRC : POS_SRC_STREAM, r.o[1])) return false;
		if (!room(pos, 1, limit)) return bad(pos, "MESH / SPLINE runs past its block");
		r.b = d.bytes[pos++];
		if (r.b > 2) return bad(at, "subindex above 2");
		if (!scalar && r.o[0].type != PS_OUT) return unsupported_form(at, "whole-chunk SPLINE into a channel or a register: the reference asserts an output");
		if (r.o[0].type == PS_CHANNEL && wmask) *wmask |= (uint16_t)(1u << r.o[0].index);
		if (is_mesh) {
			const ParticleOperand& index = r.o[1]; // written when it is negative: it counts as written
			if (index.type == PS_GLOBAL || index.type == PS_SYSTEM_VALUE) return bad(at, "MESH index is a global or a system value: it cannot take the drawn vertex");
			if (index.type == PS_LITERAL && index.value < 0.0f) return bad(at, "MESH index is a negative literal: it cannot take the drawn vertex");
			if (index.type == PS_CHANNEL && wmask) *wmask |= (uint16_t)(1u << index.index);
			r.a = at; // the byte offset: made an ordinal once every section is decoded
			++out.mesh_count;
		}
		return true;
	}
	bool unsupported_form(uint32_t at, const char* what) {
		unsupported = true;
		return bad(at, what);
	}

	// Instructions run per particle by the scalar interpreter (ParticleSystem::run) from `pos` to the END that closes them. With
	// `exact` the END must be the block's last byte (`limit`). Leaves `pos` behind the END.
	bool scalar_block(uint32_t& pos, uint32_t limit, bool exact, uint32_t depth, bool skip_pending, uint8_t end_kind, uint32_t* end_rec, uint16_t* wmask, bool* kills) {
		for (;;) {
			if (!room(pos, 1, limit)) return bad(pos, "block without its END");
			const uint32_t at = pos;
			const uint8_t op = d.bytes[pos++];
			ParticleRec r;
			memset(&r, 0, sizeof(r));
			r.op = op;
			switch (op) {
				case P_END:
					if (exact && pos != limit) return bad(at, "END before the end of its block");
					r.kind = end_kind;
					if (end_rec) *end_rec = (uint32_t)out.recs.size();
					out.recs.push_back(r);
					return true;
				case P_KILL:
					if (section != SEC_UPDATE || in_emit_block) return bad(at, "KILL outside a conditional block of the update program");
					if (kills) *kills = true;
					out.has_kill = true;
					out.recs.push_back(r);
					break;
				case P_MESH: case P_SPLINE:
					if (!source_op(op, at, pos, limit, true, r, wmask)) return false;
					if (out.stopped) return true;
					out.recs.push_back(r);
					break;
				case P_RAND:
					if (!rand_op(pos, limit, true, r, wmask)) return false;
					out.recs.push_back(r);
					break;
				case P_EMIT: {
					if (section != SEC_UPDATE || in_emit_block) return bad(at, "EMIT outside a conditional block of the update program");
					if (!room(pos, 4, limit)) return bad(at, "EMIT runs past its block");
					r.a = get<uint32_t>(pos);
					pos += 4;
					if (r.a >= d.n_emitters) return bad(at, "EMIT target out of range");
					if (depth + 1 > PARTICLE_MAX_NESTING) return bad(at, "nesting deeper than the interpreter's stack");
					if (out.emit_count >= PARTICLE_MAX_EMITS) return bad(at, "more than 8 EMIT instructions");
					r.b = out.emit_count;
					out.emit_target[out.emit_count] = r.a;
					out.emit_group[out.emit_count++] = (uint8_t)(group < 255 ? group : 255);
					out.has_emit = true;
					out.recs.push_back(r);
					in_emit_block = true; // (its own run(): a fresh skip stack)
					const bool ok = scalar_block(pos, limit, false, depth + 1, false, PE_EMIT_END, nullptr, nullptr, nullptr);
					in_emit_block = false;
					if (!ok || out.stopped) return ok;
					break;
				}
				case P_CMP: case P_CMP_ELSE: {
					if (skip_pending) return bad(at, "conditional inside the true arm of a CMP_ELSE: the interpreter's END would skip the wrong bytes");
					if (depth + 1 > PARTICLE_MAX_NESTING) return bad(at, "nesting deeper than the interpreter's stack");
					if (!operand(pos, limit, true, POS_SRC, r.o[0])) return false;
					const bool has_else = op == P_CMP_ELSE;
					if (!room(pos, has_else ? 4 : 2, limit)) return bad(at, "conditional runs past its block");
					const uint32_t ts = get<uint16_t>(pos), fs = has_else ? get<uint16_t>(pos + 2) : 0;
					pos += has_else ? 4 : 2;
					if (!room(pos, ts, limit) || !room(pos + ts, fs, limit)) return bad(at, "block size runs past the program");
					const size_t me = out.recs.size();
					out.recs.push_back(r);
					uint32_t true_end = 0;
					if (!scalar_block(pos, pos + ts, true, depth + 1, has_else, has_else ? PE_JUMP : PE_CONTINUE, &true_end, wmask, kills)) return false;
					if (out.stopped) return true;
					out.recs[me].a = (uint32_t)out.recs.size();
					if (has_else) {
						if (!scalar_block(pos, pos + fs, true, depth + 1, false, PE_CONTINUE, nullptr, wmask, kills)) return false;
						if (out.stopped) return true;
						out.recs[true_end].a = (uint32_t)out.recs.size();
					}
					break;
				}
				case P_BLEND: case P_GRADIENT:
					return bad(at, "BLEND / GRADIENT inside a conditional block: the scalar interpreter reads them as CMP_ELSE");
				default:
					if (n_sources(op) < 0) return bad(at, "instruction type out of range");
					if (!arith(op, pos, limit, true, r, wmask)) return false;
					out.recs.push_back(r);
					break;
			}
		}
	}

	// A program run over whole chunks (processChunk): the update and the output program.
	bool chunk_program(uint32_t pos) {
		const uint32_t limit = d.size;
		for (;;) {
			if (!room(pos, 1, limit)) return bad(pos, "program without its END");
			const uint32_t at = pos;
			const uint8_t op = d.bytes[pos++];
			ParticleRec r;
			memset(&r, 0, sizeof(r));
			r.op = op;
			switch (op) {
				case P_END:
					r.kind = PE_RETURN;
					out.recs.push_back(r);
					return true;
				case P_KILL: return bad(at, "KILL outside a conditional block");
				case P_EMIT: return bad(at, "EMIT outside a conditional block");
				case P_NOT: return bad(at, "NOT outside a conditional block");
				case P_MESH: case P_SPLINE:
					if (!source_op(op, at, pos, limit, false, r, nullptr)) return false;
					if (out.stopped) return true;
					out.recs.push_back(r);
					break;
				case P_RAND:
					if (!rand_op(pos, limit, false, r, nullptr)) return false;
					out.recs.push_back(r);
					break;
				case P_GRADIENT: {
					if (!operand(pos, limit, false, POS_DST, r.o[0])) return false;
					if (r.o[0].type == PS_CHANNEL) return bad(at, "GRADIENT writes outputs and registers only");
					if (!operand(pos, limit, false, POS_SRC_STREAM, r.o[1])) return false;
					if (!room(pos, 4, limit)) return bad(at, "GRADIENT runs past the program");
					const uint32_t count = get<uint32_t>(pos);
					pos += 4;
					if (count < 2 || count > PARTICLE_MAX_GRADIENT) return bad(at, "GRADIENT with fewer than 2 or more than 8 keys");
					if (!room(pos, 8 * count, limit)) return bad(at, "GRADIENT keys run past the program");
					ParticleGradient g;
					memset(&g, 0, sizeof(g));
					g.count = count;
					memcpy(g.keys, d.bytes + pos, 4 * count);
					memcpy(g.values, d.bytes + pos + 4 * count, 4 * count);
					pos += 8 * count;
					for (uint32_t i = 1; i < count; ++i) g.ms[i] = (g.values[i] - g.values[i - 1]) / (g.keys[i] - g.keys[i - 1]);
					r.a = (uint32_t)out.gradients.size();
					out.gradients.push_back(g);
					out.recs.push_back(r);
					break;
				}
				case P_CMP: case P_CMP_ELSE: {
					if (!operand(pos, limit, false, POS_SRC_STREAM, r.o[0])) return false;
					const bool has_else = op == P_CMP_ELSE;
					if (!room(pos, has_else ? 4 : 2, limit)) return bad(at, "conditional runs past the program");
					const uint32_t ts = get<uint16_t>(pos), fs = has_else ? get<uint16_t>(pos + 2) : 0;
					pos += has_else ? 4 : 2;
					if (!room(pos, ts, limit) || !room(pos + ts, fs, limit)) return bad(at, "block size runs past the program");
					const size_t me = out.recs.size();
					out.recs.push_back(r);
					uint16_t wmask = 0;
					bool kills = false;
					if (!scalar_block(pos, pos + ts, true, 1, false, PE_RETURN, nullptr, &wmask, &kills)) return false;
					if (out.stopped) return true;
					out.recs[me].a = (uint32_t)out.recs.size();
					if (has_else) {
						if (!scalar_block(pos, pos + fs, true, 1, false, PE_RETURN, nullptr, &wmask, &kills)) return false;
						if (out.stopped) return true;
					}
					++group;
					out.recs[me].c = (uint32_t)out.recs.size();
					out.recs[me].b = kills ? 1u : 0u;
					out.recs[me].wmask = kills ? wmask : 0;
					out.shadow_mask |= out.recs[me].wmask;
					break;
				}
				default:
					if (n_sources(op) < 0) return bad(at, "instruction type out of range");
					if (!arith(op, pos, limit, false, r, nullptr)) return false;
					out.recs.push_back(r);
					break;
			}
		}
	}
};

} // namespace

ParticleDecodeResult particle_program_decode(const ParticleProgramDesc& desc, ParticleProgram& out, std::string& error) {
	out = ParticleProgram();
	Decoder dec(desc, out, error);
	if (!desc.bytes || desc.size == 0) return dec.bad(0, "empty program"), PD_INVALID;
	if (desc.channels_count > PARTICLE_MAX_CHANNELS) return dec.bad(0, "more than 16 channels"), PD_INVALID;
	if (desc.registers_count > PARTICLE_MAX_REGISTERS || desc.registers_count + desc.emit_inputs_count > PARTICLE_MAX_REGISTERS) return dec.bad(0, "more than 16 registers"), PD_INVALID;
	if (desc.outputs_count > 255) return dec.bad(0, "more than 255 outputs"), PD_INVALID;
	if (desc.emit_offset >= desc.size || desc.output_offset >= desc.size) return dec.bad(0, "program offset outside the stream"), PD_INVALID;
	dec.section = SEC_UPDATE;
	out.update_at = 0;
	const auto refused = [&]() { return dec.unsupported ? PD_UNSUPPORTED : PD_INVALID; };
	if (!dec.chunk_program(0)) return refused();
	if (out.stopped) return PD_OK;
	dec.section = SEC_EMIT;
	out.emit_at = (uint32_t)out.recs.size();
	uint32_t pos = desc.emit_offset;
	if (!dec.scalar_block(pos, desc.size, false, 0, false, PE_RETURN, nullptr, nullptr, nullptr)) return refused();
	if (out.stopped) return PD_OK;
	dec.section = SEC_OUTPUT;
	out.output_at = (uint32_t)out.recs.size();
	if (!dec.chunk_program(desc.output_offset)) return refused();
	if (out.stopped) return PD_OK;
	// MESH ordinals: by byte offset, whatever order the sections lie in (the draw of a MESH does not depend on which one was decoded first)
	std::vector<uint32_t> at;
	for (const ParticleRec& r : out.recs)
		if (r.op == P_MESH) at.push_back(r.a);
	std::sort(at.begin(), at.end());
	for (ParticleRec& r : out.recs)
		if (r.op == P_MESH) r.a = (uint32_t)(std::lower_bound(at.begin(), at.end(), r.a) - at.begin());
	return PD_OK;
}

} // namespace lmx
