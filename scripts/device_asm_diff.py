"""Is the gfx950 device code of the operator translation units the same in two source trees?  (runs without a GPU)

usage: python scripts/device_asm_diff.py OTHER_TREE [file-stem ...] > profiles/rNN_device_asm.txt

Compiles dicp_amd/csrc/<stem>.hip of OTHER_TREE and of this tree with _lib.FLAGS -S --cuda-device-only and compares the assembly.  Lines
that differ between any two compilations are left out: .file / .ident and the ones naming the per-compilation symbol __hip_cuid_<hash>.
Per file: line count, function count, and "identical" or the diff.  When the whole texts differ the functions are also compared one by
one by name, which tells a changed instantiation order from changed code.  Exit status 1 if any file differs.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from dicp_amd import _lib  # noqa: E402

STEMS = ("normals", "voxel", "knn_points", "fps", "ball_query", "knn_grid", "group")
SKIP = re.compile(r"^\s*\.(file|ident)\s|__hip_cuid_")


def device_asm(tree, stem, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + _lib.FLAGS + ["-I", os.path.join(tree, "include"), "-S", "--cuda-device-only", "-o", out,
                                                  os.path.join(tree, "dicp_amd", "csrc", stem + ".hip")], stderr=subprocess.DEVNULL)
    with open(out) as f:
        return [ln for ln in f.read().splitlines() if not SKIP.search(ln)]


def functions(lines):
    """{name: its lines from the label to .Lfunc_end} of every `.type name,@function`, in file order (dicts keep it)."""
    out, name, body = {}, None, None
    for ln in lines:
        m = re.match(r"^\s*\.type\s+([^,\s]+),@function", ln)
        if m:
            name = m.group(1)
        elif name is not None and body is None and ln.startswith(name + ":"):
            body = out[name] = []
        if body is not None:
            body.append(ln)
            if ln.startswith(".Lfunc_end"):
                name = body = None
    return out


def main():
    other = os.path.abspath(sys.argv[1])
    stems = sys.argv[2:] or STEMS
    differ = False
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=4) as pool:
        jobs = {(tag, s): pool.submit(device_asm, tree, s, os.path.join(tmp, "%s_%s.s" % (tag, s)))
                for s in stems for tag, tree in (("other", other), ("this", HERE))}
        for s in stems:
            a, b = jobs["other", s].result(), jobs["this", s].result()
            fa, fb = functions(a), functions(b)
            print("%s.hip: other %d lines, %d functions; this %d lines, %d functions: %s"
                  % (s, len(a), len(fa), len(b), len(fb), "identical" if a == b else "DIFFERENT"))
            if a == b:
                continue
            differ = True
            print("  functions: names %s, order %s, bodies that differ: %s"
                  % ("equal" if set(fa) == set(fb) else "DIFFERENT", "equal" if list(fa) == list(fb) else "DIFFERENT",
                     [n for n in fa if n in fb and fa[n] != fb[n]] or "none"))
            for ln in difflib.unified_diff(a, b, "other/" + s + ".s", "this/" + s + ".s", lineterm="", n=1):
                print("  " + ln)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
