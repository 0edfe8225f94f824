"""Static per-phase instruction counts of one batched_round_kernel instantiation (CPU only).

    python tools/isa_phases.py                       # compile pcx_batched.hip, the 50 x 20 packed kernel
    python tools/isa_phases.py --kernel Li0ELi0ELb0ELb1E
    python tools/isa_phases.py --asm FILE.s          # an assembly listing made before (another revision's)
    python tools/isa_phases.py --flags=-DNAME=VALUE

Compiles pyconsensus_amd/csrc/pcx_batched.hip to gfx950 assembly with the Makefile's flags, takes
the kernel whose mangled name contains --kernel, and splits its text at the phase-stamp markers
(the shader-clock reads of the STAMP macro and of the median profile, `s_memtime`).  Per segment it
prints the instruction counts by class, told by the mnemonic's prefix alone (vector ALU `v_`, LDS
`ds_`, scalar `s_`, memory `global_` / `flat_` / `scratch_` / `buffer_`, and `s_nop` on its own),
and the lane-spill traffic: `v_writelane` stores into and `v_readlane` reloads from the VGPRs the
compiler annotates as "SGPR spill to VGPR lane" carriers.  Then the kernel's register and spill
metadata of every batched_round_kernel instantiation.

The attribution is static and approximate: segments follow the text order, not the stamp numbers;
the compiler moves code across the markers (it sank a whole accumulation from the rescale phase to
the participation phase once), loops count once whatever their trip count, and both sides of a
branch count.  The tool prints; it checks nothing.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyconsensus_amd", "csrc")
C3_KERNEL = "batched_round_kernelILi50ELi20ELb0ELb1E"
CLASSES = ("valu", "lds", "salu", "mem", "s_nop", "other")
META = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def makefile_flags():
    """CXXFLAGS of pyconsensus_amd/csrc/Makefile with its variables filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    return hipcc, flags.replace("$(ARCH)", arch).replace("$(HERE)", CSRC + os.sep).split()


def compile_asm(extra):
    hipcc, flags = makefile_flags()
    fd, out = tempfile.mkstemp(suffix=".s")
    os.close(fd)
    try:
        r = subprocess.run([hipcc] + flags + extra + ["-x", "hip", "--cuda-device-only", "-S",
                                                      os.path.join(CSRC, "pcx_batched.hip"), "-o", out],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            raise SystemExit("hipcc failed:\n" + r.stderr[-4000:])
        return open(out).read()
    finally:
        if os.path.exists(out):
            os.unlink(out)


def kernel_body(asm, key):
    """(name, instruction lines with their comments) of the kernel whose symbol contains `key`."""
    lines = asm.splitlines()
    start = name = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(\w+):", ln)
        if m and key in m.group(1) and m.group(1).startswith("_Z"):
            start, name = i + 1, m.group(1)
            break
    if start is None:
        raise SystemExit("no kernel matching %r in the listing" % key)
    body = []
    for ln in lines[start:]:
        if ln.startswith(".Lfunc_end") or ln.lstrip().startswith(".amdhsa_kernel"):
            break
        body.append(ln)
    return name, body


def classify(mn):
    if mn == "s_nop":
        return "s_nop"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "mem"
    return "other"


def segments(body):
    """Per-segment counters; a new segment starts after each s_memtime."""
    carriers = set()
    for ln in body:
        m = re.search(r"implicit-def: \$vgpr(\d+) : SGPR spill to VGPR lane", ln)
        if m:
            carriers.add("v" + m.group(1))
    segs = [dict.fromkeys(CLASSES + ("spill_st", "spill_ld", "scratch_st", "scratch_ld"), 0)]
    for ln in body:
        code = ln.split(";")[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        parts = code.replace(",", " ").split()
        mn = parts[0]
        s = segs[-1]
        s[classify(mn)] += 1
        if mn == "v_writelane_b32" and parts[1] in carriers:
            s["spill_st"] += 1
        elif mn == "v_readlane_b32" and len(parts) > 2 and parts[2] in carriers:
            s["spill_ld"] += 1
        elif mn.startswith("scratch_store"):
            s["scratch_st"] += 1
        elif mn.startswith("scratch_load"):
            s["scratch_ld"] += 1
        if mn == "s_memtime":
            segs.append(dict.fromkeys(s, 0))
    return segs, sorted(carriers, key=lambda v: int(v[1:]))


def metadata(asm):
    """{kernel symbol: {field: value}} of every batched_round_kernel in the listing's metadata."""
    out = {}
    for entry in re.split(r"^  - \.agpr_count:.*$", asm, flags=re.M)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if not m or "batched_round_kernel" not in m.group(1):
            continue
        fields = dict(re.findall(r"^    \.(\w+):\s+(\d+)\s*$", entry, re.M))
        out[m.group(1)] = {f: int(fields[f]) for f in META if f in fields}
    return out


def report(asm, key, file=sys.stdout):
    name, body = kernel_body(asm, key)
    segs, carriers = segments(body)
    p = lambda *a: print(*a, file=file)
    p("kernel %s" % name)
    p("segments %d (split at %d s_memtime markers, text order)" % (len(segs), len(segs) - 1))
    p("SGPR spill carriers: %s" % (" ".join(carriers) or "none"))
    hdr = "%4s %7s %6s %6s %5s %6s %6s | %8s %8s %8s %8s" % (
        ("seg",) + CLASSES + ("lane_st", "lane_ld", "scr_st", "scr_ld"))
    p(hdr)
    tot = dict.fromkeys(segs[0], 0)
    for i, s in enumerate(segs):
        for k in s:
            tot[k] += s[k]
        p("%4d %7d %6d %6d %5d %6d %6d | %8d %8d %8d %8d" % ((i,) + tuple(s[c] for c in CLASSES) + (
            s["spill_st"], s["spill_ld"], s["scratch_st"], s["scratch_ld"])))
    p("%4s %7d %6d %6d %5d %6d %6d | %8d %8d %8d %8d" % (("all",) + tuple(tot[c] for c in CLASSES) + (
        tot["spill_st"], tot["spill_ld"], tot["scratch_st"], tot["scratch_ld"])))
    p("metadata (every batched_round_kernel instantiation):")
    for k, v in metadata(asm).items():
        p("  %s" % k)
        p("    " + " ".join("%s=%d" % (f, v[f]) for f in META if f in v))
    return len(segs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--kernel", default=C3_KERNEL, help="substring of the kernel's mangled name")
    ap.add_argument("--asm", help="read this assembly listing instead of compiling")
    ap.add_argument("--flags", default="", help="extra compiler flags (build parameters)")
    a = ap.parse_args()
    asm = open(a.asm).read() if a.asm else compile_asm(a.flags.split())
    report(asm, a.kernel)


if __name__ == "__main__":
    main()
