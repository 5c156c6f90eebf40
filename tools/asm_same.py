"""Is the device code of the work tree the device code of REV?  The check of a refactor that must not change a kernel.

    python tools/asm_same.py REV [source.hip ...]        (default: every scaledreamer_amd/csrc/*.hip)

Every named source is compiled to device assembly twice with the CXXFLAGS of scaledreamer_amd/csrc/Makefile (isa_mix.makefile_flags,
`hipcc -S --cuda-device-only`): once from the work tree and once from REV, extracted with `git archive` into a temporary directory.
The compiler runs inside each tree's csrc with a relative file name, so no path enters the output.  Lines containing `__hip_cuid_`
(a symbol hipcc derives from the source text) are dropped and the rest is compared.  One line per source; for a source that differs,
the kernels whose text differs with both sides' register, spill, scratch and LDS figures.  Exit status 1 if any source differs."""
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix  # noqa: E402

REL = os.path.join("scaledreamer_amd", "csrc")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def device_asm(tree, name):
    """assembly of csrc/<name> of `tree` without the __hip_cuid_ lines, or None if REV has no such source"""
    csrc = os.path.join(tree, REL)
    if not os.path.exists(os.path.join(csrc, name)):
        return None
    hipcc, flags = isa_mix.makefile_flags()
    if not hipcc:
        raise FileNotFoundError("hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([hipcc] + flags + ["-w", "-S", "--cuda-device-only", "-o", out, name], cwd=csrc)
        return "".join(ln for ln in open(out) if "__hip_cuid_" not in ln)


def kernels(asm):
    """{kernel: (its text: body and kernel descriptor, {field: value} of its metadata entry)}"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    meta = {}
    for entry in re.split(r"^  - (?=\.)", asm, flags=re.M)[1:]:
        m = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if m:
            meta[m.group(1)] = {f: v for f, v in re.findall(r"^\s+(\.\w+):\s+(\S+)", entry, re.M) if f in FIELDS}
    res = {}
    for k in names:
        body = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(k), asm, re.M | re.S)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n.*?\.end_amdhsa_kernel" % re.escape(k), asm, re.M | re.S)
        res[k] = ((body.group(0) if body else "") + (desc.group(0) if desc else ""), meta.get(k, {}))
    return res


def compare(name, old, new):
    """(identical?, report lines)"""
    if old is None or new is None:
        return False, [f"{name}: only in {'the work tree' if old is None else 'REV'}"]
    if old == new:
        return True, [f"{name}: identical"]
    ko, kn = kernels(old), kernels(new)
    short = isa_mix.demangle(sorted(set(ko) | set(kn)))
    lines = []
    for k in sorted(set(ko) | set(kn)):
        to, mo = ko.get(k, ("", {}))
        tn, mn = kn.get(k, ("", {}))
        if to == tn:
            continue
        lines.append(f"    {short[k]}" + ("" if to and tn else "  (only in %s)" % ("REV" if to else "the work tree")))
        for f in FIELDS:
            lines.append(f"        {f:28s} {mo.get(f, '-'):>8s} -> {mn.get(f, '-'):>8s}")
    return False, [f"{name}: DIFFERS" + ("" if lines else " (outside the kernels)")] + lines


def main(argv):
    if not argv or argv[0].startswith("-"):
        print(__doc__)
        return 2
    rev = argv[0]
    names = sorted(os.path.basename(a) for a in argv[1:]) or sorted(f for f in os.listdir(isa_mix.CSRC) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", isa_mix.ROOT, "archive", rev, "scaledreamer_amd/csrc", "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            new = list(pool.map(lambda n: device_asm(isa_mix.ROOT, n), names))
            old = list(pool.map(lambda n: device_asm(tmp, n), names))
    same = True
    for n, o, w in zip(names, old, new):
        ok, lines = compare(n, o, w)
        same = same and ok
        print("\n".join(lines))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
