"""lumixengine_amd/host/gpu_texture_compressor.h - the texture compressor's host adapter - against the reference's REAL headers (LBCHeader,
gpu::TextureFormat, OutputMemoryStream) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h + lumix_compat_texcomp.h.
Syntax-only, as tests/test_probes_compile.py: the engine itself cannot be linked here. The first is skipped where the reference tree is
absent. TextureCompressor::Input and Options are private to the plugin's translation unit, so the input type of the first is a struct with
the members the adapter reads, over the reference's own OutputMemoryStream; the same translation unit holds the compat header's format
values and header layout to the engine's."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_texture_compressor.h"\n'
       "template <typename InputT, typename OptionsT, typename StreamT> bool use(Lumix::GpuTextureCompressor& c, const InputT& in, const OptionsT& opt, StreamT& dst) {\n"
       "\tconst bool ok = c.compress(in, opt, dst) && Lumix::GpuTextureCompressor::formatOf(in, opt) != Lumix::gpu::TextureFormat::RGBA8;\n"
       "\treturn ok && c.lastError() != nullptr && c.handle() != nullptr && Lumix::GpuTextureCompressor::mipSize(4u, 3u) == 1u;\n"
       "}\n")


def test_texture_compressor_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "texcomp_tu.cpp"
    tu.write_text('#include "core/stream.h"\n' + USE +
                  "struct Image { Lumix::OutputMemoryStream pixels; Lumix::u32 mip, face, slice; };\n"
                  "struct Input { Lumix::u32 w, h, slices, mips; bool is_srgb, is_normalmap, has_alpha, is_cubemap;\n"
                  "\tbool has(Lumix::u32, Lumix::u32, Lumix::u32) const; const Image& get(Lumix::u32, Lumix::u32, Lumix::u32) const; };\n"
                  "struct Options { bool compress = true; bool generate_mipmaps = false; };\n"
                  "template bool use<Input, Options, Lumix::OutputMemoryStream>(Lumix::GpuTextureCompressor&, const Input&, const Options&, Lumix::OutputMemoryStream&);\n"
                  "static_assert((Lumix::u32)Lumix::gpu::TextureFormat::RGBA8 == 4 && (Lumix::u32)Lumix::gpu::TextureFormat::BC1 == 15 && (Lumix::u32)Lumix::gpu::TextureFormat::BC3 == 17 &&\n"
                  "\t(Lumix::u32)Lumix::gpu::TextureFormat::BC5 == 19, \"tests/cpp/lumix_compat_texcomp.h holds other values\");\n"
                  "static_assert(sizeof(Lumix::LBCHeader) == 32 && Lumix::LBCHeader::CUBEMAP == 1, \"tests/cpp/lumix_compat_texcomp.h holds another header\");\n")
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_texture_compressor_compiles_standalone(tmp_path):
    tu = tmp_path / "texcomp_tu.cpp"
    tu.write_text(USE + "template bool use<Lumix::TexCompatInput, Lumix::TexCompatOptions, Lumix::TexCompatStream>(Lumix::GpuTextureCompressor&, const Lumix::TexCompatInput&, "
                  "const Lumix::TexCompatOptions&, Lumix::TexCompatStream&);\nstatic_assert(sizeof(Lumix::LBCHeader) == 32, \"eight words\");\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wno-multichar", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
