"""lumixengine_amd/host/gpu_probe_baker.h - the probe bake's host adapter - against the reference's REAL headers (EnvironmentProbe, Array,
Vec3, Vec4) under -DLMX_WITH_LUMIX_HEADERS, and against tests/cpp/lumix_compat.h + lumix_compat_probes.h. Syntax-only, as
tests/test_voxels_compile.py: the engine itself cannot be linked here. The first is skipped where the reference tree is absent. ProbeJob
is private to the plugin's translation unit, so the job type of the first is a struct with the members the adapter reads, over the
reference's own Array<Vec4>."""
import os
import subprocess

from tests.test_plugin_compile import FLAGS, HOST, REF, ROOT, ref_src  # noqa: F401 - ref_src is the fixture

USE = ('#include "gpu_probe_baker.h"\n'
       "template <typename JobT, typename ProbeT> bool use(Lumix::GpuProbeBaker& b, JobT* const* jobs, ProbeT* const* probes, Lumix::u8* dst) {\n"
       "\tbool ok = b.bakeEnvironment(jobs, probes, 3u) && probes[0]->sh_coefs[8].z == probes[1]->sh_coefs[0].x;\n"
       "\tok = ok && b.bakeReflection(jobs, 2u);\n"
       "\tfor (Lumix::u32 face = 0; face < 6; ++face)\n"
       "\t\tfor (Lumix::u32 mip = 0; mip < Lumix::GpuProbeBaker::LEVELS; ++mip) {\n"
       "\t\t\tconst Lumix::GpuProbeBaker::Image img = b.rgbm(1u, face, mip);\n"
       "\t\t\tmemcpy(dst, img.begin, img.bytes);\n"
       "\t\t\tok = ok && img.size != 0;\n"
       "\t\t}\n"
       "\tLmxProbesDevice d;\n"
       "\treturn ok && b.getOutputs(d) && b.lastError() != nullptr && b.handle() != nullptr && d.d_rgbm != nullptr;\n"
       "}\n")


def test_probe_baker_compiles_against_reference_headers(ref_src, tmp_path):  # noqa: F811
    tu = tmp_path / "probes_tu.cpp"
    tu.write_text('#include "core/array.h"\n' + USE + "struct Job { Lumix::Array<Lumix::Vec4> data; bool is_reflection; };\n"
                  "template bool use<Job, Lumix::EnvironmentProbe>(Lumix::GpuProbeBaker&, Job* const*, Lumix::EnvironmentProbe* const*, Lumix::u8*);\n")
    cmd = ["g++"] + FLAGS + ["-I" + ref_src, "-I" + os.path.join(REF, "external"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST, str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_probe_baker_compiles_standalone(tmp_path):
    tu = tmp_path / "probes_tu.cpp"
    tu.write_text(USE + "template bool use<Lumix::ProbeCompatJob, Lumix::ProbeCompatEnvironmentProbe>(Lumix::GpuProbeBaker&, Lumix::ProbeCompatJob* const*, "
                  "Lumix::ProbeCompatEnvironmentProbe* const*, Lumix::u8*);\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "cpp"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
