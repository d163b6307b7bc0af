"""What the tests/test_gpu_adapters_run*.py files share: building a C++ driver of tests/cpp/run_*.cpp against liblumix_mi355.so, running it on
a scenario file and reading its output file front to back."""
import os
import struct
import subprocess

import numpy as np

from lumixengine_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
HOST = os.path.join(ROOT, "lumixengine_amd", "host")
BUILD = os.path.join(ROOT, "tests", "_build")
COMMON = ["adapter_run.h", "lumix_compat.h"]
DRIVERS = {  # driver -> (the adapter headers it runs, the compat headers it fills)
    "run_instanced_models": (["gpu_instanced_models.h"], []),
    "run_cluster_filler": (["gpu_cluster_filler.h", "gpu_culling_system.h"], ["lumix_compat_lights.h"]),
    "run_grass": (["gpu_grass.h"], ["lumix_compat_grass.h"]),
    "run_ray_caster": (["gpu_ray_caster.h", "gpu_instanced_models.h"], ["lumix_compat_rays.h", "lumix_compat_scene_rays.h"]),
    "run_animators": (["gpu_animator.h", "world_sync.h"], ["lumix_compat_animator.h"]),
    "run_particles": (["gpu_particle_system.h"], ["lumix_compat_particles.h"]),
}


def library():
    """liblumix_mi355.so, built when a CPU-only run has not built it yet (the *_compiles_and_links tests link against it)"""
    from lumixengine_amd import build

    if not os.path.exists(api.LIB_PATH):
        build.build()


def build_exe(name):
    """tests/cpp/<name>.cpp -> tests/_build/<name>, rebuilt when a source it includes is newer (as build_exe() of tests/test_gpu_bridges.py)"""
    host, compat = DRIVERS[name]
    src, exe = os.path.join(CPP, name + ".cpp"), os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    deps = [src] + [os.path.join(HOST, h) for h in host] + [os.path.join(CPP, h) for h in COMMON + compat] + [os.path.join(ROOT, "include", h) for h in ("lumix_mi355.h", "lmx_types.h")]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return exe
    lib_dir = os.path.join(ROOT, "lumixengine_amd")
    tmp = f"{exe}.{os.getpid()}.tmp"  # several pytest workers may build the same driver at once: each links its own file and moves it into place
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + CPP, src, "-o", tmp, "-L" + lib_dir, "-llumix_mi355",
                    "-Wl,-rpath," + lib_dir, "-pthread"], check=True)
    os.replace(tmp, exe)
    return exe


class Out:
    """the driver's output file, read front to back"""

    def __init__(self, raw_bytes: bytes):
        self.raw, self.at = raw_bytes, 0

    def arr(self, dtype, n):
        dtype = np.dtype(dtype)
        assert self.at + n * dtype.itemsize <= len(self.raw), "the driver's output ends early"
        a = np.frombuffer(self.raw, dtype, n, self.at)
        self.at += n * dtype.itemsize
        return a

    def u32(self) -> int:
        return int(self.arr(np.uint32, 1)[0])

    def i32(self) -> int:
        return int(self.arr(np.int32, 1)[0])

    def counted(self, dtype):
        return self.arr(dtype, self.u32())

    def done(self) -> bool:
        return self.at == len(self.raw)


def run_driver(name, tmp_dir, scenario: bytes, expect_rc=0, args=()) -> Out:
    """runs the driver on `scenario`; its exit status is the step that disagreed with the scenario (tests/cpp/adapter_run.h)"""
    exe = build_exe(name)
    inp, outp = os.path.join(str(tmp_dir), name + "_in.bin"), os.path.join(str(tmp_dir), name + "_out.bin")
    with open(inp, "wb") as f:
        f.write(scenario)
    r = subprocess.run([exe, inp, outp] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == expect_rc, f"{name}: rc {r.returncode}: {r.stdout}{r.stderr}"
    with open(outp, "rb") as f:
        return Out(f.read())


def u32(*v):
    return struct.pack("<%dI" % len(v), *v)


def raw(a, dtype):
    return np.ascontiguousarray(a, dtype).tobytes()
