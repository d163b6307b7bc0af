"""GpuTextureCompressor::compressWithMips (lumixengine_amd/host/gpu_texture_compressor.h) against the reference's REAL headers (LBCHeader,
gpu::TextureFormat, OutputMemoryStream) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat_texcomp.h + lumix_compat_texmips.h.
Syntax-only, as tests/test_texcomp_compile.py: the engine itself cannot be linked here, and the first is skipped where the reference tree is
absent. TextureCompressor::Input and Options are private to the plugin's translation unit, so they are structs with the members the adapter
reads - Options with stochastic_mipmap and scale_coverage_ref as render_plugins.cpp:77-82 declares them."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_texture_compressor.h"\n'
       "template <typename InputT, typename OptionsT, typename StreamT> bool use(Lumix::GpuTextureCompressor& c, const InputT& in, const OptionsT& opt, StreamT& dst) {\n"
       "\treturn c.compressWithMips(in, opt, dst) && !c.compress(in, opt, dst) && c.lastError() != nullptr;\n"
       "}\n")


def test_compress_with_mips_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "texmips_tu.cpp"
    tu.write_text('#include "core/stream.h"\n' + USE +
                  "struct Image { Lumix::OutputMemoryStream pixels; Lumix::u32 mip, face, slice; };\n"
                  "struct Input { Lumix::u32 w, h, slices, mips; bool is_srgb, is_normalmap, has_alpha, is_cubemap;\n"
                  "\tbool has(Lumix::u32, Lumix::u32, Lumix::u32) const; const Image& get(Lumix::u32, Lumix::u32, Lumix::u32) const; };\n"
                  "struct Options { bool compress = true; bool generate_mipmaps = false; bool stochastic_mipmap = false; float scale_coverage_ref = -0.5f; };\n"
                  "template bool use<Input, Options, Lumix::OutputMemoryStream>(Lumix::GpuTextureCompressor&, const Input&, const Options&, Lumix::OutputMemoryStream&);\n")
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_compress_with_mips_compiles_standalone(tmp_path):
    tu = tmp_path / "texmips_tu.cpp"
    tu.write_text(USE + '#include "lumix_compat_texmips.h"\n'
                  "template bool use<Lumix::TexCompatInput, Lumix::TexMipsCompatOptions, Lumix::TexCompatStream>(Lumix::GpuTextureCompressor&, const Lumix::TexCompatInput&, "
                  "const Lumix::TexMipsCompatOptions&, Lumix::TexCompatStream&);\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-multichar", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
