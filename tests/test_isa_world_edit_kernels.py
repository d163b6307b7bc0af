"""The kernels of world_edit_kernels.hip as the build compiles them for gfx950 (no GPU needed: hipcc -S).

Arithmetic: k_edit_locals computes World::setParent's stored local with Transform::computeLocal and is compared bit for bit with the
reference's FMA-free fp32 / fp64, so it may not hold a fused multiply-add of its own; the only ones allowed are those of the compiler's expansions of the IEEE
divisions, recognised as the instructions between a division's v_div_scale pair and its v_div_fixup, in that division's width.

Residency: every kernel is one lane per entity, slot or list entry with a handful of indices live; none may spill. First build (VGPRs,
LDS bytes): k_edit_mark 3 / 0, k_edit_kill 6 / 0, k_edit_bury 7 / 0, k_edit_link 6 / 0, k_edit_keys 10 / 16, k_edit_child_ranges 8 / 0,
k_edit_child_counts 5 / 0, k_edit_roots 13 / 0, k_edit_level_small 22 / 16, k_edit_level_count 6 / 0, k_edit_level_scatter 16 / 0,
k_edit_permute 25 / 0, k_edit_create 28 / 0, k_edit_locals 97 / 0, k_edit_remap 8 / 0, k_edit_dropped 5 / 0, k_edit_root_sizes 10 / 0, k_edit_run_table 10 / 0;
scratch 0 everywhere. The ceilings below leave room for a compiler's mood, not for a spill (k_edit_locals holds two transforms and the
fp64 division's expansion; it runs one lane per re-parented child)."""
import re

from tests.test_isa_no_fma import FMA, isa_of, kernels
from tests.test_isa_residency import metadata, pick

SOURCE = "world_edit_kernels.hip"
OPENER = re.compile(r"\b(v_div_scale_f(32|64)|v_rcp_(iflag_)?f(32|64)|v_rsq_f(32|64)|v_sqrt_f(32|64))")
KERNELS = ("k_edit_mark", "k_edit_kill", "k_edit_bury", "k_edit_link", "k_edit_keys", "k_edit_child_ranges", "k_edit_child_counts", "k_edit_roots", "k_edit_level_small",
           "k_edit_level_count", "k_edit_level_scatter", "k_edit_permute", "k_edit_create", "k_edit_locals", "k_edit_remap", "k_edit_dropped", "k_edit_root_sizes", "k_edit_run_table")


def test_locals_have_no_fused_multiply_add_outside_division_and_root(tmp_path):
    ks = kernels(isa_of(SOURCE, tmp_path))
    bodies = [b for name, b in ks.items() if "k_edit_locals" in name]
    assert len(bodies) == 1, f"k_edit_locals not in the ISA: {list(ks)}"
    body = bodies[0]
    # An IEEE division is v_div_scale x 2 ... v_div_fmas ... v_div_fixup, with the Newton steps' FMAs in between. A fused multiply-add is
    # the expansion's only while a division is open - more v_div_scale pairs begun than v_div_fixup done - and only in that division's
    # width; rotate and qmul hold none anywhere. (Stricter than a window of instructions behind an opener: a contracted product of the
    # quaternion code that the scheduler left behind the last division would be counted here.)
    bad, scales, fixups = [], {"f32": 0, "f64": 0}, {"f32": 0, "f64": 0}
    for l in body:
        m = re.search(r"\bv_div_(scale|fixup)_(f32|f64)", l)
        if m:
            (scales if m.group(1) == "scale" else fixups)[m.group(2)] += 1
        elif FMA.search(l):
            width = "f64" if "f64" in l else "f32"
            if 2 * fixups[width] >= scales[width]:
                bad.append(l)
    assert not bad, f"k_edit_locals contains fused multiply-adds outside an open division: {bad[:5]}"
    assert scales["f64"] == 2 * fixups["f64"] and scales["f32"] == 2 * fixups["f32"] and fixups["f64"] >= 3 and fixups["f32"] >= 3, (scales, fixups)
    assert not re.search(r"\bv_(sqrt|rsq)_f(32|64)", "\n".join(body)), "computeLocal takes no root: nothing else may open an expansion"
    text = "\n".join(body)
    assert "v_div_fixup_f64" in text and "v_div_fixup_f32" in text, "computeLocal divides positions (fp64) and scales (fp32) by the parent's scale: IEEE divisions"
    assert len(re.findall(r"\bv_mul_f64", text)) >= 9 and len(re.findall(r"\bv_(pk_)?mul_f32", text)) >= 8, "rotate and qmul as separate products (16 fp32 products of qmul, two to a packed instruction at the most)"
    # the order never comes out of an atomic: the count of live entities is a sum, the list of dropped bindings a set
    for name, b in ks.items():
        atomics = [l for l in b if re.search(r"\b(global_atomic|flat_atomic|buffer_atomic|ds_add|ds_cmpst)", l)]
        assert not atomics or "k_edit_keys" in name or "k_edit_dropped" in name, (name, atomics[:3])  # (the dropped bindings are a set: the host marks them)
        assert all("atomic_add" in l for l in atomics), (name, atomics[:3])


def test_residency(tmp_path):
    meta = metadata(SOURCE, tmp_path)
    seen = {}
    for tag in KERNELS:
        (m,) = pick(meta, tag)
        seen[tag] = (m["next_free_vgpr"], m["group_segment_fixed_size"], m["private_segment_fixed_size"])
    print(seen)
    for tag, (vgpr, lds, scratch) in seen.items():
        assert scratch == 0, f"{tag} spills: {scratch} B of scratch per lane"
        assert lds == (16 if tag in ("k_edit_level_small", "k_edit_keys") else 0), (tag, lds)  # one word per wave for the block's sum
        assert vgpr <= (128 if tag == "k_edit_locals" else 64), f"{tag}: {vgpr} VGPRs"
