"""ISA comparison against another revision (no GPU needed): every kernel of the given csrc/*_kernels.hip files is compiled for gfx950
with the build's flags, once from the working tree and once from `git archive REV`, and compared - its register / scratch / LDS
metadata and its instruction sequence (comments, directives and labels stripped, label numbers blanked). One line per kernel:
    identical       the same instruction sequence
    same multiset   the same instructions in another order
    same opcodes    the same opcodes, each as often, on other registers or in another order
    differs         another set of instructions (the counts say by how much)
A change that only moves definitions must come out `identical` everywhere.
    python tools/isa_compare.py REV [file.hip ...]        (default: every csrc/*_kernels.hip)"""
import collections
import glob
import os
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lumixengine_amd import build as B  # noqa: E402
from tests.test_isa_no_fma import kernels  # noqa: E402
from tests.test_isa_residency import metadata  # noqa: E402

FIELDS = (("next_free_vgpr", "vgpr"), ("next_free_sgpr", "sgpr"), ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "lds"))


def compile_tree(tree, sources):
    """[(metadata, {kernel: normalised instructions})] of the sources of the copy of csrc/ and include/ under `tree`"""
    flags = list(B.FLAGS)
    B.FLAGS = [f.replace("-I" + ROOT, "-I" + tree) if f.startswith("-I" + ROOT) else f for f in flags]  # (metadata() compiles with B.FLAGS)

    def one(source):
        path = os.path.join(tree, "lumixengine_amd", "csrc", source)
        if not os.path.exists(path):
            return {}, {}
        meta = metadata(path, pathlib.Path(tree))  # (an absolute source: the .s is written next to it)
        text = open(os.path.splitext(path)[0] + ".s").read().splitlines()
        return meta, {k: [re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\s*;.*$", "", l)) for l in v] for k, v in kernels(text).items()}

    try:
        with ThreadPoolExecutor(max_workers=min(8, len(sources))) as ex:
            return list(ex.map(one, sources))
    finally:
        B.FLAGS = flags


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    sources = [os.path.basename(s) for s in sys.argv[2:]] or sorted(os.path.basename(p) for p in glob.glob(os.path.join(B.CSRC, "*_kernels.hip")))
    with tempfile.TemporaryDirectory() as tmp:
        there, here = os.path.join(tmp, "rev"), os.path.join(tmp, "tree")
        os.makedirs(there)
        archive = subprocess.run(["git", "-C", ROOT, "archive", rev, "lumixengine_amd/csrc", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", there], input=archive, check=True)
        shutil.copytree(B.CSRC, os.path.join(here, "lumixengine_amd", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(here, "include"))
        old, new = compile_tree(there, sources), compile_tree(here, sources)
    names = sorted({k for m, _ in old + new for k in m})
    label = {}  # the kernel's name and its integer template arguments out of the mangled one: k_cull_tile<1,4,8,8,1,0>
    for k in names:
        m = re.search(r"\d+(k_[a-z0-9_]+?)(I(?:L[ib]\d+E)+E)?(?:E|$)", k)
        label[k] = m.group(1) + ("<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">" if m.group(2) else "") if m else k

    def opcodes(body):
        return collections.Counter(l.split()[0] for l in body)

    short = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], capture_output=True, text=True).stdout.strip()
    print(f"# {short} ({rev}) -> this tree; per kernel: verdict; instructions; registers, scratch and LDS bytes")
    for source, (om, ob), (nm, nb) in zip(sources, old, new):
        for k in sorted(set(om) | set(nm)):
            if k not in om or k not in nm:
                print(f"{source} {label[k]}: only in {'this tree' if k in nm else 'the other revision'}")
                continue
            a, b = ob.get(k, []), nb.get(k, [])
            verdict = "identical" if a == b else "same multiset" if collections.Counter(a) == collections.Counter(b) else "same opcodes" if opcodes(a) == opcodes(b) else "differs"
            regs = " ".join(f"{s} {om[k].get(f)}" + ("" if om[k].get(f) == nm[k].get(f) else f" -> {nm[k].get(f)}") for f, s in FIELDS)
            print(f"{source} {label[k]}: {verdict}; instructions {len(a)}" + ("" if len(a) == len(b) else f" -> {len(b)}") + f"; {regs}")


if __name__ == "__main__":
    main()
