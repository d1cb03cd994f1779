#!/usr/bin/env python3
"""Are the full-call kernels of csrc/qpn_verify.hip the code they were before the list form?  Compiles the unit of
this tree and of another checkout (the parent commit) to gfx950 code objects with the flags of csrc/build.sh, disassembles both
and compares, kernel by kernel, the instruction words of the <LIST = false> instantiations with the parent's kernels of the
same name (the parent has no LIST argument).  Needs no GPU.  Usage: python tools/verify_fullcall_disasm.py PARENT_CHECKOUT"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = os.path.join("quadraticprogramnetworks.jl_amd", "csrc", "qpn_verify.hip")
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
tmp = tempfile.mkdtemp()


def kernels(tree, tag):
    """{demangled kernel name without the LIST argument: [instruction text + encoding, ...]} of one tree's code object"""
    co = os.path.join(tmp, tag + ".co")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall",
                           "-Wno-unused-parameter", "--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(tree, REL), "-o", co])
    dis = subprocess.run([OBJDUMP, "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::|^void ", "", name).split("(")[0]
            cur = out.setdefault(name, [])
            continue
        m = re.match(r"^\s+(\S.*?)\s*// [0-9A-F]+: ([0-9A-F ]+)", line)
        if m and cur is not None:
            cur.append((m.group(1), m.group(2).strip()))
    return out


def full_call_name(name):
    """this tree's name of a full-call instantiation -> the parent's name of the same kernel, None for a list instantiation"""
    m = re.match(r"^(\w+)<(.*)>$", name)
    if not m:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    if args[-1] != "false":
        return None
    return m.group(1) + ("<" + ", ".join(args[:-1]) + ">" if len(args) > 1 else "")


old, new = kernels(sys.argv[1], "parent"), kernels(ROOT, "this")
bad = 0
for name in sorted(new):
    was = full_call_name(name)
    if was is None:
        continue
    same = was in old and old[was] == new[name]
    bad += not same
    print(f"{'identical' if same else 'DIFFERENT':9s}  {name:40s} {len(new[name]):6d} instructions   (parent: {was}"
          f"{', %d' % len(old[was]) if was in old else ', missing'})")
missing = [k for k in old if k not in {full_call_name(n) for n in new}]
if missing:
    print("parent kernels without a full-call counterpart:", missing)
sys.exit(1 if bad or missing else 0)
