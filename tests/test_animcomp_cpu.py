"""The animation compressor's arithmetic on the host (lmx_animcomp_compress_host, csrc/lmx_animcomp.h) against tests/animcomp_oracle.py, byte
for byte: the info, the four tables and both streams of every clip of tests/animcomp_cases.py, the refusals and their codes. Each one-rule
mutant of the oracle changes a byte of some case, so the cases tell the rules apart. The header's host code also runs in a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/cpp/animcomp_host_sanitize.cpp)."""
import os

import numpy as np
import pytest

from tests import animcomp_cases as AC
from tests import animcomp_oracle as AO

GOOD = [c["name"] for c in AC.good_clips()]
REFUSED = [(c["name"], status) for c, status in AC.refused_clips()]
# the cases that tell each rule: a mutant must change a byte of at least one of them
MUTANT_CASES = {
    "tie_later": ("zeros in different waves of a workgroup, 1 bone", "zeros in different workgroups, 1 bone", "zeros in different workgroups, 40 bones", "zeros in one workgroup, 40 bones"),
    "no_half": ("ties at k + 0.5",), "pack_fp32": ("frame of 57 bits",), "pow2": ("frame of 7 bits",), "clamp_from_1": ("clamp, one largest",),
    "skip_last_largest": ("clamp, four equal sizes",), "sign_le": ("clamp, four equal sizes",), "bind_ge": ("at the bind error exactly",),
    "offsets_all_tracks": ("63 samples, 64 bones",)}


@pytest.fixture(scope="module")
def api():
    from lumixengine_amd import api

    return api


@pytest.mark.parametrize("name", GOOD)
def test_host_equals_oracle(api, name):
    got, want = api.animcomp_compress_host(AC.by_name(name)), AC.want(name)
    assert want["status"] == AO.OK, f"{name}: the oracle refuses it with {want['status']}"
    assert not AO.differences(got, want), f"{name}: " + "; ".join(AO.differences(got, want))


def test_cases_reach_what_they_are_for():
    """the shapes the issue lists, read off the oracle's results"""
    w = AC.want
    assert w("frame of 4 bits")["rotations_frame_size_bits"] == 4 and w("frame of 4 bits")["rotations"]["bitsizes"].tolist() == [[1, 1, 1]]
    for bits in (7, 37, 57, 64, 65, 2280):
        assert w(f"frame of {bits} bits")["translations_frame_size_bits"] == bits
    offsets = set()
    for c in AC.good_clips():
        if c["name"].startswith("57 bits at offset"):
            t = w(c["name"])["translations"][-1]
            assert t["bitsizes"].sum() == 57
            offsets.add(int(t["offset_bits"]) & 7)
    assert offsets == set(range(8))
    for name, lo_sign, hi_sign in (("zeros in different waves of a workgroup, 1 bone", True, False), ("zeros in different workgroups, 1 bone", False, True),
                                   ("zeros in different workgroups, 40 bones", True, False), ("zeros in one workgroup, 40 bones", False, True)):
        t = w(name)["translations"][0]
        assert t["min"][0] == 0 and bool(np.signbit(t["min"][0])) == lo_sign, name  # x: the minimum is the earlier zero
        assert t["min"][1] < 0 and t["bone_index"] == 0
        later = AC.want(name, "tie_later")["translations"][0]
        assert bool(np.signbit(later["min"][0])) != lo_sign
    z = w("a zero-range channel in an animated track")
    assert z["translations"][0]["bitsizes"].tolist() == [7, 1, 7] and z["translations"][0]["to_range"][1] == 0
    assert w("clamp, four equal sizes")["rotations"]["bitsizes"].tolist() == [[16, 16, 16]] and w("clamp, four equal sizes")["rotations"]["skipped_channel"][0] == 0
    one = w("clamp, one largest")["rotations"][0]
    assert one["skipped_channel"] == 0 and one["bitsizes"].tolist() == [15, 16, 16]
    assert w("rotation sizes of 64 in all")["rotations"]["bitsizes"].tolist() == [[16, 16, 16]]
    assert w("leaves the bind pose in its last sample")["n_const_translations"] == 1 and w("stays within the bind pose")["n_const_translations"] == 0
    assert w("at the bind error exactly")["n_const_translations"] == 0
    forced = [t for c in AC.good_clips() if c["name"].endswith("bones") for t in w(c["name"])["translations"] if (t["bitsizes"] == 1).any() and (t["to_range"] > 0).all()]
    assert forced, "a range of bit size 0 forced to 1"
    ts = np.unpackbits(w("frame of 7 bits")["translation_stream"], bitorder="little")[: 7 * 33].reshape(33, 7)
    x = ts[:, 0] + 2 * ts[:, 1]
    assert 0 in x and 3 in x, "keys at the minimum and the maximum: fields 0 and 2^b - 1"


def test_fixture_of_the_reference_equals_oracle_and_host(api):
    """tests/golden/animcomp_small.npz: the reference's own bytes of a handful of clips, from the translation count on (recorded by
    tests/golden/make_golden_animcomp.py; tests/test_animcomp_oracle_vs_ref.py checks that the reference still gives them). Stands where the
    reference tree is absent."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "animcomp_small.npz"))
    hashes = (np.arange(1, 197, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)
    assert len(g["names"]) >= 8
    for i, name in enumerate(str(n) for n in g["names"]):
        c = AC.by_name(name)
        assert np.array_equal(AC.as_floats(c["keys"]).view(np.uint32), g[f"keys_{i}"].view(np.uint32)) and np.array_equal(c["bind"], g[f"bind_{i}"]), f"{name}: the generator no longer makes the recorded clip"
        for what, result in (("the oracle", AC.want(name)), ("the host entry", api.animcomp_compress_host(c))):
            section = AO.ani_file(result, hashes, "", 30.0, 0)[8 + 1 + 12:]
            assert section == g[f"bytes_{i}"].tobytes(), f"{name}: {what} against the reference's recorded bytes"


@pytest.mark.parametrize("name,status", REFUSED)
def test_refusals(api, name, status):
    got, want = api.animcomp_compress_host(AC.by_name(name)), AC.want(name)
    assert want["status"] == status, f"{name}: the oracle says {want['status']}"
    assert not AO.differences(got, want), f"{name}: " + "; ".join(AO.differences(got, want))


def test_undefined_cases_follow_the_contract(api):
    """a zero-range channel packs the field 0 and nothing leaves the entry; log2 of 0 is 0; a non-finite bind position without keys is not looked at"""
    z = api.animcomp_compress_host(AC.by_name("a zero-range channel in an animated track"))
    bits = np.unpackbits(z["translation_stream"], bitorder="little")[: 24 * 33].reshape(33, 24)
    assert not bits[:, 7].any(), "the y field of the first track"
    assert bits[:, :7].any() and bits[:, 8:15].any()
    name = "a NaN bind position of a bone without keys"
    got = api.animcomp_compress_host(AC.by_name(name))
    assert got["status"] == AO.OK and not AO.differences(got, AC.want(name))
    one = api.animcomp_compress_host(AC.by_name("1 sample"))
    assert one["n_translations"] == 0 and one["n_rotations"] == 0 and one["n_const_rotations"] == 3 and one["frame_count"] == 0


def test_malformed_descriptors(api):
    c = dict(AC.by_name("2 samples"))
    c["keys"] = np.zeros((2, 197), api.ANIM_KEY)
    c["bind"] = np.zeros((197, 3), np.float32)
    with pytest.raises(api.LumixError) as e:
        api.animcomp_compress_host(c)
    assert e.value.code == 1


@pytest.mark.parametrize("rule", AO.MUTANTS)
def test_mutant_changes_a_byte(rule):
    assert set(MUTANT_CASES) == set(AO.MUTANTS)
    changed = [name for name in MUTANT_CASES[rule] if (AO.flat(AC.want(name, rule)).tobytes() != AO.flat(AC.want(name)).tobytes())]
    assert changed, f"no case tells the rule '{rule}'"
    if rule == "tie_later":
        assert len(changed) == len(MUTANT_CASES[rule]), "every order and place of the two zeros tells it"


def test_host_arithmetic_runs_clean_under_sanitizers(tmp_path):
    """csrc/lmx_animcomp.h as host code - whole clips at the edges of the bit layout, the refusals, the last byte of a stream - in a
    stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer"""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "animcomp_host_sanitize"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "lumixengine_amd", "csrc"), os.path.join(root, "tests", "cpp", "animcomp_host_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
