// controller_fuzz.cpp — stand-alone driver of the controller parser and the host build of the controller VM (lmx_controller_program.{h,cpp}),
// built by tests/test_controller_program.py with -fsanitize=address,undefined. For every valid stream of the input file: every truncation
// and every single-bit flip is parsed from a heap copy of its exact size (a read past the stream is a sanitizer report). What the parser
// accepts is run: the enter image, then eight updates with two time steps, in buffers of exactly the bounds the parser computed - the
// runtime-data words, the instruction records, the pose stack - so a bound that is too small is a sanitizer report too.
//
// First of all ctl_fmod1 is held against fmodf(x, 1) on two million bit patterns and the edge values.
//
// input file: u32 n_streams, then per stream u32 size + bytes. Prints "<n> accepted, <m> refused".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lmx_controller_program.h"

using namespace lmx;

static bool run_program(const ControllerProgram& p) {
	// one synthetic clip in every slot: 4 frames at 30 fps with both root-motion arrays
	const uint32_t frames = 4;
	std::vector<float> rm_t(3 * (frames + 1)), rm_r(4 * (frames + 1));
	for (uint32_t f = 0; f <= frames; ++f) {
		rm_t[3 * f] = 0.125f * f; rm_t[3 * f + 1] = 0.f; rm_t[3 * f + 2] = -0.25f * f;
		rm_r[4 * f] = 0.f; rm_r[4 * f + 1] = 0.6f; rm_r[4 * f + 2] = 0.f; rm_r[4 * f + 3] = 0.8f;
	}
	const CtlClip clip = {30.f, frames, 4369u, 0u, 0u};
	std::vector<uint32_t> slots(p.n_slots, 0u), ik_leaf(p.ik_bones.size(), LMX_BONE_NONE);
	std::vector<uint32_t> inputs(4 * p.input_types.size());
	for (size_t i = 0; i < p.input_types.size(); ++i) {
		inputs[4 * i] = p.input_types[i];
		inputs[4 * i + 1] = p.input_types[i] == LMX_VALUE_BOOL ? (uint32_t)(i & 1) : ctl_u(0.75f * (float)(i + 1));
		inputs[4 * i + 2] = inputs[4 * i + 3] = ctl_u(0.5f);
	}
	// exact-size heap buffers (a std::vector's capacity may exceed its size)
	std::unique_ptr<uint32_t[]> a(new uint32_t[p.state_words ? p.state_words : 1]), b(new uint32_t[p.state_words ? p.state_words : 1]);
	std::unique_ptr<LmxBlendInstr[]> instrs(new LmxBlendInstr[p.max_instrs ? p.max_instrs : 1]);
	std::unique_ptr<CtlFrame[]> stack(new CtlFrame[LMX_CONTROLLER_MAX_POSE_DEPTH]);
	if (p.enter_image.size() > p.state_words) return false;
	memcpy(a.get(), p.enter_image.data(), 4 * p.enter_image.size());
	uint32_t len = (uint32_t)p.enter_image.size();
	Rigid root_motion = Rigid{V3{0, 0, 0}, Q4{0, 0, 0, 1}};
	for (int frame = 0; frame < 8; ++frame) {
		CtlCtx c = {};
		c.nodes = p.nodes.data(); c.ops = p.ops.data(); c.exprs = p.exprs.data(); c.aux = p.aux.data();
		c.slots = slots.data(); c.clips = &clip; c.rm_t = rm_t.data(); c.rm_r = rm_r.data();
		c.inputs = inputs.data(); c.ik_leaf = ik_leaf.data();
		c.in = a.get(); c.out = b.get(); c.stride = 1;
		c.time_delta = frame & 1 ? 546u : 3000u;
		c.weight = 1.f;
		c.root_motion = root_motion;
		c.instrs = instrs.get();
		ctl_update(c, p.root, stack.get());
		if (c.rd != len || c.wr > p.state_words || c.n_instrs > p.max_instrs) return false; // the update reads exactly what the last one wrote
		len = c.wr;
		root_motion = c.root_motion;
		a.swap(b);
		if (frame == 3) // flip the inputs: transitions start
			for (size_t i = 0; i < p.input_types.size(); ++i) inputs[4 * i + 1] = p.input_types[i] == LMX_VALUE_BOOL ? (uint32_t)(~i & 1) : ctl_u(2.f - 0.5f * (float)i);
	}
	return true;
}

static int try_stream(const uint8_t* bytes, size_t n, size_t& accepted, size_t& refused) {
	std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
	if (n) memcpy(copy.get(), bytes, n);
	ControllerProgram p;
	std::string error;
	if (!controller_program_parse(n ? copy.get() : nullptr, n, p, error)) {
		++refused;
		return 0;
	}
	++accepted;
	if (!run_program(p)) {
		fprintf(stderr, "an accepted program left its bounds\n");
		return 1;
	}
	return 0;
}

// fmodf(x, 1) is exact by definition; so must its restatement be, bit for bit, the sign of a zero included (NaN for NaN)
static int check_fmod1() {
	const float edges[] = {0.f, -0.f, 1.f, -1.f, 2.f, -2.f, 0.5f, -0.5f, 1.5f, -1.5f, 0.99999994f, 1.00000012f, 8388607.5f, -8388607.5f, 8388608.f, 16777216.f, -16777216.f,
		1.4e-45f, -1.4e-45f, 1.17549435e-38f, 3.4e38f, -3.4e38f, INFINITY, -INFINITY, NAN};
	uint32_t seed = 12345u;
	for (uint32_t k = 0; k < (1u << 21) + sizeof(edges) / sizeof(edges[0]); ++k) {
		float x;
		if (k < sizeof(edges) / sizeof(edges[0])) x = edges[k];
		else {
			seed = seed * 1664525u + 1013904223u;
			x = ctl_f(seed);
		}
		const float a = ctl_fmod1(x), b = fmodf(x, 1.f);
		if (std::isnan(a) != std::isnan(b) || (!std::isnan(a) && ctl_u(a) != ctl_u(b))) {
			fprintf(stderr, "fmod1(%a) = %a, fmodf gives %a\n", (double)x, (double)a, (double)b);
			return 1;
		}
	}
	return 0;
}

int main(int argc, char** argv) {
	if (argc < 2) return 2;
	if (check_fmod1()) return 1;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint32_t n_streams = 0;
	if (fread(&n_streams, 4, 1, f) != 1) return 2;
	size_t accepted = 0, refused = 0;
	for (uint32_t s = 0; s < n_streams; ++s) {
		uint32_t size = 0;
		if (fread(&size, 4, 1, f) != 1) return 2;
		std::vector<uint8_t> bytes(size);
		if (size && fread(bytes.data(), 1, size, f) != size) return 2;
		size_t ok_before = accepted;
		if (try_stream(bytes.data(), size, accepted, refused)) return 1;
		if (accepted == ok_before) {
			fprintf(stderr, "valid stream %u was refused\n", s);
			return 1;
		}
		for (size_t cutoff = 0; cutoff < size; ++cutoff)
			if (try_stream(bytes.data(), cutoff, accepted, refused)) return 1;
		for (size_t bit = 0; bit < 8 * (size_t)size; ++bit) {
			bytes[bit / 8] ^= (uint8_t)(1u << (bit % 8));
			const int rc = try_stream(bytes.data(), size, accepted, refused);
			bytes[bit / 8] ^= (uint8_t)(1u << (bit % 8));
			if (rc) return 1;
		}
	}
	fclose(f);
	printf("%zu accepted, %zu refused\n", accepted, refused);
	return 0;
}
