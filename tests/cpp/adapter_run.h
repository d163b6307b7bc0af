// adapter_run.h — what the run_*.cpp drivers of the engine-facing adapters share: a scenario file read front to back, an output file
// written front to back, and the exit codes. A scenario is a stream of little-endian records its pytest wrote (tests/test_gpu_adapters_run*.py);
// a record that expects `true` from an adapter call and gets `false` (or the reverse) ends the driver with that step's exit code and the
// adapter's lastError() on stderr.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace adapter_run {

enum { EXIT_USAGE = 2, EXIT_NO_DEVICE = 3, EXIT_SCENARIO = 9, EXIT_STEP = 10 }; // a failed step k exits with EXIT_STEP + its op code

struct Reader {
	std::vector<uint8_t> bytes;
	size_t at = 0;
	bool open(const char* path) {
		FILE* f = fopen(path, "rb");
		if (!f) return false;
		fseek(f, 0, SEEK_END);
		const long n = ftell(f);
		fseek(f, 0, SEEK_SET);
		bytes.resize(n > 0 ? (size_t)n : 0);
		const bool ok = bytes.empty() || fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
		fclose(f);
		return ok;
	}
	bool done() const { return at >= bytes.size(); }
	void need(size_t n) {
		if (at + n > bytes.size()) { fprintf(stderr, "scenario: %zu bytes wanted at %zu of %zu\n", n, at, bytes.size()); exit(EXIT_SCENARIO); }
	}
	template <typename T> T get() {
		T v;
		need(sizeof(T));
		memcpy(&v, bytes.data() + at, sizeof(T));
		at += sizeof(T);
		return v;
	}
	template <typename T> std::vector<T> arr(size_t n) {
		std::vector<T> v(n);
		need(n * sizeof(T));
		if (n) memcpy(static_cast<void*>(v.data()), bytes.data() + at, n * sizeof(T));
		at += n * sizeof(T);
		return v;
	}
};

struct Writer {
	FILE* f = nullptr;
	bool open(const char* path) { return (f = fopen(path, "wb")) != nullptr; }
	template <typename T> void put(const T& v) { fwrite(&v, sizeof(T), 1, f); }
	template <typename T> void arr(const T* p, size_t n) {
		if (n) fwrite(p, sizeof(T), n, f);
	}
	template <typename T> void counted(const std::vector<T>& v, size_t n) { // u32 n, then n records
		put((uint32_t)n);
		arr(v.data(), n);
	}
	void close() {
		if (f) fclose(f);
		f = nullptr;
	}
};

// the step `op` answered `got` where the scenario says `want`
inline void expect(bool got, bool want, uint32_t op, const char* what, const char* error) {
	if (got == want) return;
	fprintf(stderr, "step %u (%s): returned %s, the scenario expects %s: %s\n", op, what, got ? "true" : "false", want ? "true" : "false", error ? error : "");
	exit(EXIT_STEP + (int)op);
}

} // namespace adapter_run
