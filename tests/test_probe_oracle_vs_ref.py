"""Pins tests/probe_oracle.py to the reference's own code (CPU; skipped where the reference tree is absent).

At test time the SphericalHarmonics struct (renderer/editor/render_plugins.cpp:476-587) and the five RGBM lines of saveCubemap's loop
(:3555-3559) are cut out of the reference by anchors, placed into a harness in a temporary directory and compiled with g++, core/math.cpp
and the flags of tests/test_im_oracle_vs_ref.py. Nothing of the reference is committed. The `downscale` program (:2850-2898) is HLSL
inside a string: its loop is restated in the harness, and the test asserts that the reference still holds those lines.

The oracle is held to the reference bit for bit on every SH case of probe_oracle.cases(), on every mip of the cases that have a chain,
and on the RGBM bytes of a table of clamp routes (negative channels, m below 1 / 64 and above 4, rounding ties).
tests/golden/make_golden_probes.py records tests/golden/probes_small.npz with the same harness; a test checks that the committed
fixture is what the reference gives. The last test prints the reference's single-thread time of SphericalHarmonics::compute at S = 128.

data/shaders/ibl_filter.hlsl (from SAMPLE_COUNT on) and D_GGX (common.hlsli:764-769) are compiled as C++ against a small float2 / float3 /
float4 shim written here, with sampleCubeBindlessLod replaced by a recorder of (L, lod): the oracle's per-sample values agree with the
recorder's within stated bounds (libm and numpy differ in sin / cos / log2, and the shim's literals are doubles), the gate decisions are
identical, and lmx_probes_ggx_samples agrees with ImportanceSampleGGX's own H. What the sampler returns for (L, lod) is this library's
definition and has no reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import probe_oracle as PO
from tests.test_im_oracle_vs_ref import FLAGS, REF, _block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probes_small.npz")

HARNESS = r"""
#include <math.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "core/core.h"
#include "core/math.h"
#include "core/span.h"
#define PROFILE_FUNCTION()
using namespace Lumix;

@SH_STRUCT@

struct Rgbm { u8 r, g, b, a; };
static void encode(const Vec4* mip_pixels, Rgbm* rgbm, u32 c) {
	for (u32 j = 0; j < c; ++j) {
@RGBM_LINES@
	}
}

// the `downscale` program's main (:2862-2872) for one texel and u_scale = (2, 2)
static Vec4 downscale(const Vec4* src, int src_w, int tx, int ty) {
	const int scale_x = 2, scale_y = 2;
	Vec4 accum(0.f);
	for (int j = 0; j < scale_y; ++j) {
		for (int i = 0; i < scale_x; ++i) {
			Vec4 v = src[(tx * scale_x + i) + (ty * scale_y + j) * src_w];
			accum += v;
		}
	}
	accum *= float(1.0 / (scale_x * scale_y));
	return accum;
}

int main(int argc, char** argv) {
	FILE* f = fopen(argv[2], "rb");
	FILE* o = fopen(argv[3], "wb");
	u32 n = 0;
	if (fread(&n, 4, 1, f) != 1) return 2;
	std::vector<Vec4> px(n, Vec4(0.f));
	if (n && fread(px.data(), sizeof(Vec4), n, f) != n) return 2;
	if (!strcmp(argv[1], "sh")) {
		SphericalHarmonics sh;
		const auto t0 = std::chrono::steady_clock::now();
		sh.compute(Span<const Vec4>(px.data(), n));
		if (argc > 4) fprintf(stderr, "compute %lld\n", (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
		fwrite(sh.coefs, sizeof(Vec3), 9, o);
	} else if (!strcmp(argv[1], "rgbm")) {
		std::vector<Rgbm> out(n);
		encode(px.data(), out.data(), n);
		fwrite(out.data(), 4, n, o);
	} else { // "mip": n = 6 s^2 texels of one cubemap; one level down
		u32 s = 1;
		while (6 * s * s < n) ++s;
		for (u32 face = 0; face < 6; ++face)
			for (u32 y = 0; y < s / 2; ++y)
				for (u32 x = 0; x < s / 2; ++x) {
					const Vec4 v = downscale(px.data() + face * s * s, (int)s, (int)x, (int)y);
					fwrite(&v, sizeof(Vec4), 1, o);
				}
	}
	fclose(o);
	return 0;
}
"""

RGBM_FIRST = "const float m = clamp(maximum(mip_pixels[j].x, mip_pixels[j].y, mip_pixels[j].z), 1 / 64.f, 4.f);"
RGBM_LAST = "rgbm[j].a = u8(clamp(255.f * m / 4 + 0.5f, 1.f, 255.f));"
DOWNSCALE_LINES = ("float4 accum = 0;", "for (int j = 0; j < cb.u_scale.y; ++j) {", "for (int i = 0; i < cb.u_scale.x; ++i) {",
                   "float4 v = bindless_textures[cb.u_src][thread_id.xy * cb.u_scale + int2(i, j)];", "accum += v;", "accum *= 1.0 / (cb.u_scale.x * cb.u_scale.y);",
                   "bindless_rw_textures[cb.u_dst][thread_id.xy] = accum;", "m_model_plugin.downscale(stream, mip_views[mip - 1], mip_size << 1, mip_size << 1, mip_views[mip], mip_size, mip_size);")


def build_harness(d):
    """compiles the cut pieces of the reference into `d` (a directory outside the repository) -> the executable"""
    d = str(d)
    src = os.path.join(REF, "src")
    core = os.path.join(d, "core")
    shutil.copytree(os.path.join(src, "core"), core)
    sync = os.path.join(core, "sync.h")
    if os.path.exists(sync):
        open(sync, "w").write(open(sync).read().replace('#error "Not implemented"', "pthread_rwlock_t lock;", 1))
    rp = open(os.path.join(src, "renderer", "editor", "render_plugins.cpp")).read()
    sh = "struct SphericalHarmonics {" + _block(rp, "struct SphericalHarmonics") + "};"
    for line in ("const float u = (x + 0.5f) / w;", "const float temp = 1.0f + u * u + v * v;", "const float weight = 4.0f / (sqrtf(temp) * temp);", "v *= -1.f;",
                 "*this += project(dir) * (color * weight);", "*this = *this * ((4.0f * PI) / weightSum);", "case 3: return normalize(Vec3(u, -1.f, v));", "0.488603f * 2 / 3.f,"):
        assert line in sh, line
    a, b = rp.index(RGBM_FIRST), rp.index(RGBM_LAST) + len(RGBM_LAST)
    lines = rp[a:b]
    assert lines.count("\n") == 4 and "rgbm[j].r = u8(clamp(mip_pixels[j].x / m * 255 + 0.5f, 0.f, 255.f));" in lines, lines
    for line in DOWNSCALE_LINES:
        assert line in rp, line
    open(os.path.join(d, "harness.cpp"), "w").write(HARNESS.replace("@SH_STRUCT@", sh).replace("@RGBM_LINES@", lines))
    stubs = os.path.join(d, "stubs.cpp")
    open(stubs, "w").write('#include "core/os.h"\nnamespace Lumix::os { u64 Timer::getRawTimestamp() { return 1; } }\n')
    inc = ["-I" + d, "-I" + src, "-I" + os.path.join(REF, "external")]
    objs = []
    for path in (os.path.join(d, "harness.cpp"), stubs, os.path.join(core, "math.cpp")):
        obj = os.path.join(d, os.path.basename(path) + ".o")
        r = subprocess.run(["g++"] + FLAGS + inc + ["-c", path, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = os.path.join(d, "probes_ref")
    r = subprocess.run(["g++"] + FLAGS + objs + ["-o", exe, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_ref(ref, mode, texels, time=False):
    """texels: float32 (k, 4) through one mode of the harness -> (the raw output, stderr)"""
    exe, d = ref
    t = np.ascontiguousarray(texels, np.float32).reshape(-1, 4)
    open(os.path.join(d, "job.bin"), "wb").write(np.uint32(len(t)).tobytes() + t.tobytes())
    r = subprocess.run([exe, mode, os.path.join(d, "job.bin"), os.path.join(d, "out.bin")] + (["time"] if time else []), check=True, timeout=300, capture_output=True, text=True)
    return open(os.path.join(d, "out.bin"), "rb").read(), r.stderr


def ref_sh(ref, cubemap):
    return np.frombuffer(run_ref(ref, "sh", cubemap)[0], "<f4").reshape(9, 3).copy()


def ref_mips(ref, cubemap):
    out, a = [], np.ascontiguousarray(cubemap, np.float32)
    while a.shape[1] > 1:
        s = a.shape[1] // 2
        a = np.frombuffer(run_ref(ref, "mip", a)[0], "<f4").reshape(6, s, s, 4).copy()
        out.append(a)
    return out


def ref_rgbm(ref, texels):
    t = np.asarray(texels, np.float32)
    return np.frombuffer(run_ref(ref, "rgbm", t)[0], np.uint8).reshape(t.shape[:-1] + (4,)).copy()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.isdir(os.path.join(REF, "src")):
        pytest.skip("no reference tree on this machine")
    d = tmp_path_factory.mktemp("probes_ref")
    return build_harness(d), str(d)


@pytest.mark.parametrize("name", list(PO.cases()))
def test_sh_oracle_matches_the_reference(ref, name):
    c = PO.cases()[name]
    for p, cubemap in enumerate(c["cubemaps"]):
        got, want = PO.sh_compute(cubemap), ref_sh(ref, cubemap)
        assert got.tobytes() == want.tobytes(), f"{name} probe {p}: {np.nonzero(got.view(np.uint32) != want.view(np.uint32))} {got.reshape(-1)[:4]} vs {want.reshape(-1)[:4]}"


@pytest.mark.parametrize("name", [k for k, c in PO.cases().items() if c["mips"]])
def test_mip_oracle_matches_the_downscale_loop(ref, name):
    for p, cubemap in enumerate(PO.cases()[name]["cubemaps"]):
        got, want = PO.mip_chain(cubemap), ref_mips(ref, cubemap)
        assert len(got) == len(want)
        for m, (a, b) in enumerate(zip(got, want)):
            assert a.tobytes() == b.tobytes(), f"{name} probe {p} mip {m + 1}"


def test_rgbm_oracle_matches_savecubemap(ref):
    rng = np.random.default_rng(5)
    texels = np.concatenate([PO.rgbm_routes().reshape(-1, 4), np.concatenate([(10.0 ** rng.uniform(-4, 1.5, (4000, 3))).astype(np.float32), np.ones((4000, 1), np.float32)], axis=1)])
    got, want = PO.rgbm_texels(texels), ref_rgbm(ref, texels)
    assert got.tobytes() == want.tobytes(), np.nonzero((got != want).any(axis=1))[0][:10]
    assert want[:, 3].min() == 1 and want[:, 3].max() == 255 and (want[:, :3] == 0).any() and (want[:, :3] == 255).any()
    assert PO.rgbm_texels(texels, {"rgbm_without_half"}).tobytes() != want.tobytes()


def test_golden_fixture_is_what_the_reference_gives(ref):
    """tests/golden/probes_small.npz (made by tests/golden/make_golden_probes.py) still holds the reference's outputs of every case"""
    from tests.golden.make_golden_probes import recorded

    g = np.load(GOLDEN)
    want = recorded(ref)
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        if k.endswith("|e32"):  # the oracle's own float32 noise: numpy's libm may differ between machines, the figures stay the recorded ones
            assert g[k].shape == v.shape and (g[k] > 0).all() and (g[k] < 1e-2).all(), k
        else:
            assert g[k].dtype == v.dtype and g[k].tobytes() == v.tobytes(), k


def test_reference_time_of_sh_compute(ref, capsys):
    """the CPU side of DESIGN.md §4.22: SphericalHarmonics::compute on one 6 x 128 x 128 capture, single thread. A figure, no bar."""
    cubemap = PO.cases()["sh S=128 n=1"]["cubemaps"][0]
    times = []
    for _ in range(5):
        err = run_ref(ref, "sh", cubemap, time=True)[1]
        times.append(int(err.split()[1]))
    with capsys.disabled():
        print(f"\nreference, one thread, S = 128: SphericalHarmonics::compute {min(times) / 1e6:.2f} ms (best of 5)")
    assert min(times) > 0


# ---- data/shaders/ibl_filter.hlsl and D_GGX, compiled as C++ -----------------------------------------------------------------------------------
# What stands in for HLSL is a float2 / float3 / float4 with the operators the shader uses and float versions of its intrinsics; the
# shader's literals are C++ doubles here, so some of its products are rounded later than a shader compiler would round them.
# sampleCubeBindlessLod is a recorder of (L, lod); the colour it returns is 1, so mainPS returns totalWeight / totalWeight.
HLSL_SHIM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#undef M_PI
#define M_PI 3.14159265359
namespace hlsl {
typedef unsigned uint;
struct float2 { float x, y; float2() : x(0), y(0) {} float2(float a, float b) : x(a), y(b) {} };
inline float2 operator*(float2 a, float s) { return float2(a.x * s, a.y * s); }
inline float2 operator-(float2 a, float s) { return float2(a.x - s, a.y - s); }
struct float3 { float x, y, z; float3() : x(0), y(0), z(0) {} float3(float s) : x(s), y(s), z(s) {} float3(float a, float b, float c) : x(a), y(b), z(c) {} };
inline float3 operator+(float3 a, float3 b) { return float3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline float3 operator-(float3 a, float3 b) { return float3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline float3 operator*(float3 a, float s) { return float3(a.x * s, a.y * s, a.z * s); }
inline float3 operator*(float s, float3 a) { return float3(s * a.x, s * a.y, s * a.z); }
inline float3 operator/(float3 a, float s) { return float3(a.x / s, a.y / s, a.z / s); }
inline float3& operator+=(float3& a, float3 b) { a = a + b; return a; }
struct float4 { float x, y, z, w; float4(float3 v, float s) : x(v.x), y(v.y), z(v.z), w(s) {} };
inline float dot(float3 a, float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float3 cross(float3 a, float3 b) { return float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline float sqrt(float v) { return sqrtf(v); }
inline float cos(float v) { return cosf(v); }
inline float sin(float v) { return sinf(v); }
inline float log2(float v) { return log2f(v); }
inline float abs(float v) { return fabsf(v); }
inline float max(float a, float b) { return a > b ? a : b; }
inline float min(float a, float b) { return a < b ? a : b; }
inline float clamp(float v, float lo, float hi) { return min(max(v, lo), hi); }
inline float3 normalize(float3 v) { return v * (1.0f / sqrtf(dot(v, v))); }
float u_filter_roughness; int u_face; int u_mip; int u_texture; int LinearSampler;
struct Texel { float3 rgb; };
struct Record { float3 L; float lod; };
std::vector<Record> records;
inline Texel sampleCubeBindless(int, int, float3) { Texel t; t.rgb = float3(1.f); return t; }
inline Texel sampleCubeBindlessLod(int, int, float3 L, float lod) { Record r; r.L = L; r.lod = lod; records.push_back(r); Texel t; t.rgb = float3(1.f); return t; }
@D_GGX@
@IBL_FILTER@
} // namespace hlsl

int main(int argc, char** argv) {
	using namespace hlsl;
	FILE* o = fopen(argv[2], "wb");
	if (argv[1][0] == 'h') { // ImportanceSampleGGX at N = +z: its frame is tangent (0, -1, 0), bitangent (1, 0, 0), so the result is (H.y, -H.x, H.z) of the tangent-space H
		for (int level = 0; level < 5; ++level)
			for (uint i = 0; i < SAMPLE_COUNT; ++i) {
				const float3 h = ImportanceSampleGGX(Hammersley(i, SAMPLE_COUNT), float3(0.f, 0.f, 1.f), float(level) / 4);
				const float t[3] = {-h.y, h.x, h.z};
				fwrite(t, 4, 3, o);
			}
	} else { // every texel of levels 1 .. 4 of a cubemap of size S = argv[3]: per texel the number of recorded samples, then (L, lod) each
		const int S = atoi(argv[3]);
		for (u_mip = 1; u_mip < 5; ++u_mip) {
			const int s = S >> u_mip;
			u_filter_roughness = float(u_mip) / (5 - 1); // :3711
			for (u_face = 0; u_face < 6; ++u_face)
				for (int y = 0; y < s; ++y)
					for (int x = 0; x < s; ++x) {
						records.clear();
						const float4 c = mainPS(float2((x + 0.5f) / s, 1.f - (y + 0.5f) / s)); // mainVS flips pos.y: row y of the target has in_uv.y = 1 - (y + 0.5) / s
						const uint n = (uint)records.size();
						fwrite(&n, 4, 1, o);
						fwrite(&c.x, 4, 1, o);
						if (n) fwrite(records.data(), sizeof(Record), n, o);
					}
		}
	}
	fclose(o);
	return 0;
}
"""


@pytest.fixture(scope="module")
def shader(tmp_path_factory):
    shaders = os.path.join(REF, "data", "shaders")
    if not os.path.isdir(shaders):
        pytest.skip("no reference tree on this machine")
    d = str(tmp_path_factory.mktemp("probes_hlsl"))
    ibl = open(os.path.join(shaders, "ibl_filter.hlsl")).read()
    common = open(os.path.join(shaders, "common.hlsli")).read()
    assert "#define M_PI 3.14159265359" in common and "pos.y = -pos.y;" in ibl and "float dim = 128;" in ibl
    body = ibl[ibl.index("static const uint SAMPLE_COUNT = 128u;"):]
    head = "float4 mainPS(float2 in_uv : TEXCOORD0) : SV_TARGET {"
    assert head in body
    body = body.replace(head, "float4 mainPS(float2 in_uv) {", 1)
    anchor = "float D_GGX(float ndoth, float roughness)"
    d_ggx = anchor + " {" + _block(common, anchor) + "}"
    assert "float f = max(1e-5, (ndoth * ndoth) * (a2 - 1) + 1);" in d_ggx
    open(os.path.join(d, "shader.cpp"), "w").write(HLSL_SHIM.replace("@D_GGX@", d_ggx).replace("@IBL_FILTER@", body))
    exe = os.path.join(d, "shader")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-msse2", "-mfpmath=sse", "-ffp-contract=off", "-fno-fast-math", "-w", os.path.join(d, "shader.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, d


def test_ggx_sample_table_matches_the_shader(shader):
    """The oracle's table and lmx_probes_ggx_samples against ImportanceSampleGGX's own H. The bound: `1 - cosTheta * cosTheta` cancels, so an
    ulp of cosTheta (2^-24) moves sinTheta - and with it H.x and H.y - by up to cosTheta / sinTheta ulps; the shim's double literals round
    Xi.y and cosTheta's quotient once where float32 rounds twice. Eight such steps are allowed, plus 2^-21 for phi: an angle in [4, 8) has
    an ulp of 2^-21 / 2 ... 2^-21, and `2.0 * M_PI * Xi.x` is rounded to float twice in float32 and once here. H.z itself stays within 4 ulp."""
    from lumixengine_amd import api, build

    if not os.path.exists(api.LIB_PATH):
        build.build()
    exe, d = shader
    subprocess.run([exe, "h", os.path.join(d, "h.bin")], check=True, timeout=60)
    want = np.fromfile(os.path.join(d, "h.bin"), "<f4").reshape(5, 128, 3)
    for level in range(5):
        for name, got in (("oracle", PO.ggx_samples(level)), ("lmx_probes_ggx_samples", api.probes_ggx_samples(level))):
            z = want[level][:, 2].astype(np.float64)
            sin_t = np.sqrt(np.maximum(1 - z * z, 2.0 ** -40))
            bound = 8 * 2.0 ** -24 * np.maximum(z / sin_t, 1.0) + 2.0 ** -21
            err = np.abs(got.astype(np.float64) - want[level])
            assert (err[:, 2] <= 4 * 2.0 ** -24).all(), (name, level, err[:, 2].max())
            ok = (err[:, :2] <= np.minimum(bound, 1e-3)[:, None]) | (sin_t < 1e-3)[:, None]  # (sample 0 is the pole: sinTheta = 0 on both sides)
            assert ok.all(), (name, level, err[:, :2].max(), np.nonzero(~ok))


def test_filter_samples_match_the_shader(shader):
    """Every texel of levels 1 .. 4 at S = 16: the gate decisions are the shader's (the same number of samples per texel reaches the
    fetch, and they are the same samples: their L agree). L agrees with the recorder's within 1e-5 absolute (the table's bound above
    carried through the frame, on unit vectors). The lod is worse conditioned: D_GGX's `f = NdotH^2 * (a2 - 1) + 1` cancels down to a2 =
    (level / 4)^4 at NdotH = 1, so eight ulps of NdotH^2 are 8 * 2^-24 / a2 of f, twice that of f * f, and log2(e) / 2 times that of
    the lod: 1.8e-4 at level 1, 1.1e-5 at level 2, below 1e-5 beyond; 1e-5 is allowed on top for the rest of the expression."""
    exe, d = shader
    S = 16
    subprocess.run([exe, "s", os.path.join(d, "s.bin"), str(S)], check=True, timeout=120)
    raw = np.fromfile(os.path.join(d, "s.bin"), "<f4")
    at, worst_l, texels, gated = 0, 0.0, 0, 0
    for level in range(1, 5):
        s = S >> level
        face, y, x = (v.reshape(-1) for v in np.meshgrid(np.arange(6), np.arange(s), np.arange(s), indexing="ij"))
        N = PO._norm(PO.texel_dir(x, y, face, s), np.float32)
        L, ndotl, lod, gate = PO.filter_samples(tuple(v[:, None] for v in N), PO.ggx_samples(level), level, S)
        lod_bound, worst_lod = 1e-5 + 1.4427 * 8 * 2.0 ** -24 / (level / 4.0) ** 4, 0.0
        for t in range(len(x)):
            n = int(raw[at:at + 1].view(np.uint32)[0])
            assert abs(raw[at + 1] - 1.0) < 1e-6  # totalWeight / totalWeight
            rec = raw[at + 2: at + 2 + 4 * n].reshape(n, 4)
            at += 2 + 4 * n
            k = np.nonzero(gate[t])[0]
            assert len(k) == n, f"level {level} texel {t}: {len(k)} samples pass the oracle's gate, {n} the shader's"
            mine = np.stack([L[0][t, k], L[1][t, k], L[2][t, k]], axis=1)
            worst_l = max(worst_l, float(np.abs(mine - rec[:, :3]).max()))
            worst_lod = max(worst_lod, float(np.abs(lod[t, k] - rec[:, 3]).max()))
            texels += 1
            gated += n
        print(f"\nlevel {level}: |dlod| <= {worst_lod:.2e} (bound {lod_bound:.2e})")
        assert worst_lod <= lod_bound, (level, worst_lod, lod_bound)
    assert at == len(raw) and texels == 6 * (64 + 16 + 4 + 1) and 0 < gated < 128 * texels
    print(f"{texels} texels, {gated} samples: |dL| <= {worst_l:.2e}")
    assert worst_l <= 1e-5
