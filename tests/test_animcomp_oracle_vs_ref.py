"""Pins tests/animcomp_oracle.py to the reference's own clip writer (CPU; skipped where the reference tree is absent).

A harness is written at test time in a temporary directory around three pieces cut out of renderer/editor/model_importer.cpp by their anchor
lines - the helper block (BitWriter, the track structs, the packs, clampBitsizes), isBindPosePositionTrack, and the body of write_animation
from `all_keys` to the last bit_writer.write - nothing of them is committed. The harness supplies what they lean on: m_out_file (a stream
with eight bytes of slack behind it, which BitWriter's 8-byte store needs), m_bones, write, fillTracks, Array, BoneNameHash (the name is the
hash's decimal digits) and an ASSERT that counts. Vec3, Quat, Matrix, minimum and maximum are the reference's core/math.h and core/math.cpp,
linked; every bone is a root, so its bind position is its matrix's translation. Flags: -O2 -msse2 -mfpmath=sse -ffp-contract=off.

The oracle's .ani bytes from the translation count on must equal the reference's bit for bit on every generated clip, none left out: the
generator stays inside the domain where the reference is defined - in every animated track each channel has a non-zero range, no quotient
reaches 2^32, no channel exceeds 30 bits, no entry 57 - which the test asserts of each clip from the oracle's own result, as it asserts that
the reference's ASSERTs never fire. One more thing the reference leaves to chance shows only here: a bone skipped by the bind-pose test
is still packed, as an entry of 0 bits from a track whose min and max were never written (see the harness); the library skips such a bone.
The cases the reference leaves undefined are held to the oracle's stated definitions in
tests/test_animcomp_cpu.py, not here. tests/golden/animcomp_small.npz (tests/golden/make_golden_animcomp.py) holds a handful of clips and
the reference's bytes; the test checks that the reference still produces it."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import animcomp_cases as AC
from tests import animcomp_oracle as AO

REF = "/root/reference"
IMPORTER = os.path.join(REF, "src", "renderer", "editor", "model_importer.cpp")
MATH = os.path.join(REF, "src", "core", "math.cpp")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "animcomp_small.npz")
FLAGS = ["-std=c++20", "-O2", "-msse2", "-mfpmath=sse", "-ffp-contract=off", "-w", "-DNDEBUG"]
F = np.float32

pytestmark = pytest.mark.skipif(not os.path.exists(IMPORTER) or not os.path.exists(MATH) or shutil.which("g++") is None, reason="needs the reference tree and g++")

# what the cut-out pieces lean on, restated just far enough for them to compile
PRELUDE = r"""
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "core/math.h"
#include "core/os.h"
#include "core/span.h"
Lumix::u64 Lumix::os::Timer::getRawTimestamp() { return 0; } // (math.cpp's unseeded generators want it; nothing here calls them)
static int g_asserts = 0;
#undef ASSERT
#define ASSERT(x) do { if (!(x)) ++g_asserts; } while (0)
namespace Harness {
using namespace Lumix;
struct IAllocator {};
struct OutputMemoryStream {
	std::vector<u8> bytes = std::vector<u8>(8);
	u64 used = 0;
	u64 size() const { return used; }
	void resize(u64 n) { bytes.resize(n + 8); used = n; } // eight bytes of slack behind the stream
	u8* getMutableData() { return bytes.data(); }
	void write(const void* p, u64 n) { const u64 at = used; resize(used + n); memcpy(bytes.data() + at, p, n); }
	void clear() { used = 0; }
};
template <typename T> struct Array {
	std::vector<T> v;
	explicit Array(IAllocator&) {}
	u32 size() const { return (u32)v.size(); }
	bool empty() const { return v.empty(); }
	T& operator[](u32 i) { return v[i]; }
	const T& operator[](u32 i) const { return v[i]; }
	T* begin() { return v.data(); }
	T* end() { return v.data() + v.size(); }
	const T* begin() const { return v.data(); }
	const T* end() const { return v.data() + v.size(); }
};
struct BoneNameHash {
	explicit BoneNameHash(const char* name) : hash(strtoull(name, nullptr, 10)) {}
	u64 hash;
};
struct Animation { enum class TrackType : u8 { CONSTANT, ANIMATED }; };
template <typename... A> void logWarning(A&&...) {}
struct ModelImporter {
	struct Key { Vec3 pos; Quat rot; };
	struct Bone { u64 parent_id = 0; Matrix bind_pose_matrix; std::string name; };
};
"""

MAIN = r"""
using Key = ModelImporter::Key;
using Bone = ModelImporter::Bone;
struct Meta { float anim_translation_error, anim_rotation_error; };
struct Anim {};
static IAllocator m_allocator;
static OutputMemoryStream m_out_file;
static std::vector<Bone> g_bones;
struct Bones {
	u32 size() const { return (u32)g_bones.size(); }
	const Bone* begin() const { return g_bones.data(); }
	const Bone* end() const { return g_bones.data() + g_bones.size(); }
	const Bone& operator[](u32 i) const { return g_bones[i]; }
} m_bones;
static std::vector<std::vector<Key>> g_keys;
static int getParentIndex(const Bones&, const Bone&) { return 0; } // (every bone is a root)
template <typename T> static void write(const T& v) { m_out_file.write(&v, sizeof(v)); }
static void fillTracks(const Anim&, Array<Array<Key>>& all_keys, u32 from_sample, u32 samples_count) {
	all_keys.v.assign(g_keys.size(), Array<Key>(m_allocator));
	for (size_t b = 0; b < g_keys.size(); ++b) all_keys.v[b].v = g_keys[b];
}
static void write_animation(const Anim& anim, const Meta& meta, u32 from_sample, u32 samples_count) {
	const char* src = "harness";
	Array<TranslationTrack> translation_tracks(m_allocator);
	Array<RotationTrack> rotation_tracks(m_allocator);
	translation_tracks.v.resize(m_bones.size());
	rotation_tracks.v.resize(m_bones.size());
	// A bone the bind-pose test skips keeps a default TranslationTrack: not constant, three sizes of 0, min and max never written. The stream
	// loop still packs it - an entry of 0 bits whose value is u64((v - min) / (max - min) * 0 + 0.5): 0 for any finite min != max, and a NaN's
	// conversion (bit 63, ORed into a later entry where the cursor is byte-aligned) where the memory happens to hold min == max. The engine's
	// Array leaves that memory as it finds it; here it is given finite, distinct values: the reading under which the reference is defined.
	for (TranslationTrack& t : translation_tracks.v) { t.min = Vec3(0, 0, 0); t.max = Vec3(1, 1, 1); }
	m_out_file.clear();
	// ---- the reference's lines ----
@BODY@
	// ---- end ----
}
} // namespace Harness

// in: u32 clips; per clip u32 bones, samples; float t_error, r_error; per bone: u64 hash, u32 has_keys, float bind[3], then samples x 7 floats
// out: per clip u32 asserts, u64 bytes, the bytes; stderr: the loop's time
int main(int argc, char** argv) {
	using namespace Harness;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	u32 clips = 0;
	if (!in || !out || fread(&clips, 4, 1, in) != 1) return 2;
	double seconds = 0;
	for (u32 c = 0; c < clips; ++c) {
		u32 nb, ns;
		Meta meta;
		if (fread(&nb, 4, 1, in) != 1 || fread(&ns, 4, 1, in) != 1 || fread(&meta, 8, 1, in) != 1) return 3;
		g_bones.assign(nb, Bone());
		g_keys.assign(nb, {});
		for (u32 b = 0; b < nb; ++b) {
			u64 hash; u32 has; float bind[3];
			if (fread(&hash, 8, 1, in) != 1 || fread(&has, 4, 1, in) != 1 || fread(bind, 4, 3, in) != 3) return 4;
			g_bones[b].name = std::to_string(hash);
			g_bones[b].bind_pose_matrix = Matrix::IDENTITY;
			g_bones[b].bind_pose_matrix.setTranslation(Vec3(bind[0], bind[1], bind[2]));
			if (!has) continue;
			g_keys[b].resize(ns);
			for (u32 s = 0; s < ns; ++s) {
				float k[7];
				if (fread(k, 4, 7, in) != 7) return 5;
				g_keys[b][s].pos = Vec3(k[0], k[1], k[2]);
				g_keys[b][s].rot = Quat(k[3], k[4], k[5], k[6]);
			}
		}
		g_asserts = 0;
		const auto t0 = std::chrono::steady_clock::now();
		write_animation(Anim(), meta, 0, ns);
		seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		const u32 asserts = (u32)g_asserts;
		const u64 bytes = m_out_file.size();
		fwrite(&asserts, 4, 1, out);
		fwrite(&bytes, 8, 1, out);
		fwrite(m_out_file.getMutableData(), 1, bytes, out);
	}
	fclose(out);
	fprintf(stderr, "%.6f\n", seconds * 1e3);
	return 0;
}
"""


def _between(text, first, behind):
    """the lines from the one that holds `first` up to, not including, the one that holds `behind`"""
    a = text.rindex("\n", 0, text.index(first)) + 1
    b = text.rindex("\n", 0, text.index(behind, a)) + 1
    return text[a:b]


def build_harness(work):
    text = open(IMPORTER).read()
    helpers = _between(text, "struct BitWriter {", "} // anonymous namespace")
    bind_test = _between(text, "static bool isBindPosePositionTrack(", "static const ModelImporter::Bone* getParent(")
    body = _between(text, "Array<Array<Key>> all_keys(m_allocator);", "Path anim_path(name")
    src = os.path.join(work, "animcomp_harness.cpp")
    with open(src, "w") as f:
        f.write("\n".join([PRELUDE, helpers, bind_test, MAIN.replace("@BODY@", body)]))
    exe = os.path.join(work, "animcomp_harness")
    subprocess.run(["g++"] + FLAGS + ["-I" + os.path.join(REF, "src"), src, MATH, "-o", exe], check=True)
    return exe


def ref_run(exe, work, clips, hashes):
    """clips: tests/animcomp_cases dicts -> ([(asserts, bytes)], the loops' milliseconds)"""
    blob = struct.pack("<I", len(clips))
    for c in clips:
        k = AC.as_floats(c["keys"])
        ns, nb = k.shape[:2]
        has = np.ones(nb, np.uint8) if c["has_keys"] is None else c["has_keys"]
        blob += struct.pack("<IIff", nb, ns, c["translation_error"], c["rotation_error"])
        for b in range(nb):
            blob += struct.pack("<QI", int(hashes[b]), int(has[b])) + c["bind"][b].tobytes() + (np.ascontiguousarray(k[:, b]).tobytes() if has[b] else b"")
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, src, dst], check=True, capture_output=True, text=True)
    raw, at, out = open(dst, "rb").read(), 0, []
    for _ in clips:
        asserts, n = struct.unpack_from("<IQ", raw, at)
        out.append((asserts, raw[at + 12: at + 12 + n]))
        at += 12 + n
    assert at == len(raw)
    return out, float(r.stderr.strip().splitlines()[-1])


HASHES = (np.arange(1, 197, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)  # any 196 distinct numbers below 2^63
UNDEFINED = ("a zero-range channel in an animated track",)  # held to the oracle's own definition in tests/test_animcomp_cpu.py


def in_domain(want):
    """the reference is defined on this clip: read off the oracle's own result"""
    return (want["status"] == AO.OK and (want["translations"]["to_range"] != 0).all() and (want["rotations"]["to_range"] != 0).all()
            and (np.isfinite(want["translations"]["to_range"])).all())


def section(want, nb):
    """the oracle's .ani bytes from the translation count on"""
    whole = AO.ani_file(want, HASHES[:nb], "", 30.0, 0)
    return whole[8 + 1 + 12:]


def generated():
    """every good clip of tests/animcomp_cases.py but the undefined one (its shapes are the issue's list), all inside the domain"""
    return [c for c in AC.good_clips() if c["name"] not in UNDEFINED]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("animcomp_ref"))
    return build_harness(work), work


def test_oracle_equals_the_reference_on_every_generated_clip(ref):
    exe, work = ref
    clips = generated()
    assert len(clips) == len(AC.good_clips()) - len(UNDEFINED)
    got, ms = ref_run(exe, work, clips, HASHES)
    print(f"the reference's loop, one thread, {len(clips)} clips: {ms:.3f} ms")
    for c, (asserts, theirs) in zip(clips, got):
        want = AC.want(c["name"])
        assert in_domain(want), f"{c['name']}: outside the domain where the reference is defined"
        assert asserts == 0, f"{c['name']}: {asserts} of the reference's ASSERTs fired"
        ours = section(want, c["keys"].shape[1])
        assert ours == theirs, f"{c['name']}: {len(ours)} vs {len(theirs)} bytes, first difference at {next((i for i, (a, b) in enumerate(zip(ours, theirs)) if a != b), None)}"


def test_importer_sized_clip_and_the_loops_time(ref):
    """one clip of 60 bones and 300 samples of smooth curves (tools/animcomp_time.py's shape, other keys): bit for bit, and the time of the
    reference's own loop on one thread of this CPU, printed for DESIGN.md §4.25 (no bar)"""
    exe, work = ref
    c = AC.mixed("importer-sized", 300, 60, 61)
    want = AO.compress(AC.as_floats(c["keys"]), c["bind"], c["has_keys"])
    assert in_domain(want)
    best = 1e9
    for _ in range(3):
        got, ms = ref_run(exe, work, [c], HASHES)
        best = min(best, ms)
    assert got[0][0] == 0 and got[0][1] == section(want, 60)
    print(f"the reference's loop, one thread, 1 clip of 60 bones x 300 samples: {best:.3f} ms")


def test_fixture_is_what_the_reference_gives(ref):
    exe, work = ref
    g = np.load(GOLDEN)
    names = [str(n) for n in g["names"]]
    clips = [AC.by_name(n) for n in names]
    got, _ = ref_run(exe, work, clips, HASHES)
    for i, (c, (asserts, theirs)) in enumerate(zip(clips, got)):
        assert asserts == 0
        assert np.array_equal(AC.as_floats(c["keys"]), g[f"keys_{i}"]) and np.array_equal(c["bind"], g[f"bind_{i}"]), f"{names[i]}: the generator no longer makes the recorded clip"
        assert theirs == g[f"bytes_{i}"].tobytes(), names[i]
