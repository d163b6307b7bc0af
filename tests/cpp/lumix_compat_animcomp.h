// lumix_compat_animcomp.h — what lumixengine_amd/host/gpu_animation_compressor.h reads of the engine in a standalone build: Animation's
// header, version and track type (animation/animation.h:56-84; tests/test_animcomp_compile.py holds the values to the engine's where the
// reference tree exists), the bone name hash as the 64 bits the file stores (core/hash.h:44-76), and key arrays shaped like the
// importer's Array<Array<Key>> (model_importer.h), over std::vector.
#pragma once

#include <string.h>

#include <vector>

#include "lumix_compat.h"

namespace Lumix {

struct Animation {
	static const u32 HEADER_MAGIC = 0x5f4c4146; // '_LAF'
	enum class TrackType : u8 { CONSTANT, ANIMATED };
	enum class Version : u32 { COMPRESSION = 6, SKELETON, LAST };
	struct Header {
		u32 magic;
		Version version;
	};
};

struct BoneNameHash { // StableHash: the file holds getHashValue()'s 8 bytes
	static BoneNameHash fromU64(uint64_t hash) { BoneNameHash h; h.hash = hash; return h; }
	uint64_t getHashValue() const { return hash; }
private:
	uint64_t hash = 0;
};
static_assert(sizeof(BoneNameHash) == 8, "written as it is");

struct AnimCompatKey { // ModelImporter::Key
	Vec3 pos;
	Quat rot;
};
struct AnimCompatKeys { // Array<Key>
	std::vector<AnimCompatKey> v;
	size_t size() const { return v.size(); }
	bool empty() const { return v.empty(); }
	const AnimCompatKey& operator[](size_t i) const { return v[i]; }
};
struct AnimCompatAllKeys { // Array<Array<Key>>
	std::vector<AnimCompatKeys> v;
	size_t size() const { return v.size(); }
	const AnimCompatKeys& operator[](size_t i) const { return v[i]; }
};

struct AnimCompatStream { // OutputMemoryStream's members the adapter calls
	std::vector<u8> bytes;
	void write(const void* p, size_t n) {
		const size_t at = bytes.size();
		bytes.resize(at + n);
		if (n) memcpy(bytes.data() + at, p, n);
	}
	size_t size() const { return bytes.size(); }
	void resize(size_t n) { bytes.resize(n); }
};

} // namespace Lumix
