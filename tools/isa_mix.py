"""Instruction mix of the kernels of one .hip source, read from the device assembly the library's own flags produce.

    python tools/isa_mix.py scaledreamer_amd/csrc/nn_ops.hip [--kernel REGEX] [--loops] [--json]

The source is compiled with the CXXFLAGS of scaledreamer_amd/csrc/Makefile (`hipcc -S --cuda-device-only`), every kernel is split
into basic blocks at its labels, and a loop is the span between a label and a later branch back to it.  Per kernel, and for its
largest loop (most instructions; --loops lists all), the counts that tell an HBM-bound streaming pass from a VALU-bound one:
VALU instructions, v_exp / v_rcp / v_div_scale (a v_div_scale pair is one IEEE-rounded fp32 division, ~10 VALU), packed fp32,
branches, global loads and stores.  The library is built without fast-math, so `a / b` in a kernel is such a division unless the
source says __builtin_amdgcn_rcpf: this is the check that found them in the GroupNorm passes.
tests/test_isa_divides_cpu.py runs it on nn_ops.hip and gemm.hip."""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scaledreamer_amd", "csrc")
COUNTS = ("insts", "valu", "v_exp", "v_rcp", "v_div_scale", "v_pk_f32", "mfma", "salu", "branch", "loads", "stores", "lds")


def makefile_flags():
    """(hipcc, flags) from the library's Makefile: the variables HIPCC, ARCH and CXXFLAGS, nothing else is read."""
    var = {}
    for ln in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", ln)
        if m:
            var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"]).split()
    hipcc = os.environ.get("HIPCC") or var.get("HIPCC", "hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    return hipcc, flags


def device_asm(src):
    hipcc, flags = makefile_flags()
    if not hipcc:
        raise FileNotFoundError("hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([hipcc] + flags + ["-w", "-S", "--cuda-device-only", "-I", CSRC, "-o", out, os.path.abspath(src)])
        return open(out).read()


def _short_name(n):
    """name and integer template arguments of a mangled kernel the demangler at hand does not know (_Float16 arguments)"""
    m = re.match(r"_Z(\d+)", n)
    if not m:
        return n
    a = m.end()
    name, rest = n[a:a + int(m.group(1))], n[a + int(m.group(1)):]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    return name + ("<" + ", ".join(re.findall(r"L[ib](\d+)E", t.group(1))) + ">" if t else "")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if tool and names else []
    if len(out) != len(names):
        out = list(names)
    return {n: _short_name(o) if o.startswith("_Z") else o for n, o in zip(names, out)}


def classify(op):
    c = {"insts": 1}
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        c["mfma"] = 1
    elif op.startswith("v_"):
        c["valu"] = 1
        for k in ("v_exp", "v_rcp", "v_div_scale"):
            if op.startswith(k + "_"):
                c[k] = 1
        if re.match(r"v_pk_(fma|mul|add)_f32", op):
            c["v_pk_f32"] = 1
    elif op.startswith("s_cbranch") or op == "s_branch":
        c["branch"] = 1
    elif op.startswith("s_"):
        c["salu"] = 1
    elif re.match(r"(global|buffer|flat|scratch)_load", op):
        c["loads"] = 1
    elif re.match(r"(global|buffer|flat|scratch)_(store|atomic)", op):
        c["stores"] = 1
    elif op.startswith("ds_"):
        c["lds"] = 1
    return c


def tally(ops):
    t = dict.fromkeys(COUNTS, 0)
    for op in ops:
        for k, v in classify(op).items():
            t[k] += v
    return t


def analyse_asm(asm):
    """{demangled kernel name: {"total": counts, "loops": [{"label", counts...}], "main_loop": counts or None}}"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, body = {}, None, []
    for ln in asm.splitlines():
        m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in kernels:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.(Lfunc_end\d+:|end_amdhsa_kernel|section)", ln) or ln.startswith(".Lfunc_end"):
            res[cur] = body
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            body.append(("label", m.group(1)))
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        body.append(("op", parts[0], parts[1] if len(parts) > 1 else ""))
    names = demangle(sorted(res))
    out = {}
    for k, body in res.items():
        ops = [b[1] for b in body if b[0] == "op"]
        pos, loops = {}, []
        for i, b in enumerate(body):
            if b[0] == "label":
                pos[b[1]] = i
            elif b[1].startswith("s_cbranch") or b[1] == "s_branch":
                tgt = b[2].strip()
                if tgt in pos:   # a branch back to a label already seen closes a loop
                    t = tally([x[1] for x in body[pos[tgt]:i + 1] if x[0] == "op"])
                    t["label"] = tgt
                    t["blocks"] = sum(1 for x in body[pos[tgt]:i + 1] if x[0] == "label")
                    loops = [x for x in loops if x["label"] != tgt] + [t]   # several back edges to one header: the widest span
        main = max(loops, key=lambda t: t["insts"]) if loops else None
        out[names[k]] = {"mangled": k, "total": tally(ops), "loops": loops, "main_loop": main}
    return out


def analyse(src):
    return analyse_asm(device_asm(src))


def _row(name, t):
    return f"{name[:58]:58s}" + "".join(f"{t[k]:>7d}" for k in COUNTS)


def main(argv):
    if not argv or argv[0].startswith("-"):
        print(__doc__)
        return 2
    pat = re.compile(argv[argv.index("--kernel") + 1]) if "--kernel" in argv else None
    res = analyse(argv[0])
    if pat:
        res = {k: v for k, v in res.items() if pat.search(k)}
    if "--json" in argv:
        print(json.dumps(res, indent=1))
        return 0
    print(f"{'kernel / loop':58s}" + "".join(f"{k[:6]:>7s}" for k in COUNTS))
    for k in sorted(res):
        short = re.sub(r"\(.*", "", k.replace("void ", ""))
        print(_row(short, res[k]["total"]))
        loops = res[k]["loops"] if "--loops" in argv else ([res[k]["main_loop"]] if res[k]["main_loop"] else [])
        for t in loops:
            tag = "main loop" if t is res[k]["main_loop"] else "loop"
            print(_row(f"    {tag} {t['label']} ({t['blocks']} blocks)", t))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
