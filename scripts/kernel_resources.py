#!/usr/bin/env python3
"""Resource figures of the kernels of a built libfistr_hip.so, from the metadata the compiler writes into the gfx950 code object:
VGPRs (arch + accumulation), SGPRs, LDS bytes, scratch bytes, spills, and the waves per SIMD the VGPR count allows (512 registers
per lane and SIMD on gfx950, granules of 8, at most 8 waves).

    scripts/kernel_resources.py frontistr_amd/libfistr_hip.so [--filter k_nl_] [--against other/libfistr_hip.so]

Every kernel of the library is listed, so new ones need no entry here: `--filter k_heat` gives the six instantiations of the heat
conduction element kernel (fx_heat.h; the table of DESIGN.md section 4) and, as `k_heat_face` / `k_heat_bf`, the kernels of its
surface terms (fx_heat_bc.h), `--filter k_nl_` the nonlinear element kernels, `--filter k_nodal` the kernels of the nodal stress
output (fx_nodal_stress.h: `k_nodal_element<ETYPE>`, `k_nodal_node`, `k_nodal_tensor_post`), `--filter k_dload` the kernels of the
distributed loads (fx_dload.h: `k_dload_face<3 | 4 | 6 | 8>`, `k_dload_vol<ETYPE>`).

With --against: the kernels of both libraries side by side, `same` / `differs` / `new` / `gone` per kernel -- the way to show that
a change left the existing instantiations alone.  With --code as well, `same` also requires the same instruction text: the
disassembly of the kernel (llvm-objdump) without addresses and encodings and without the padding behind its last instruction; the
last line counts the kernels of the older library whose instructions are identical in the newer one.  Needs ROCm's llvm-objcopy, clang-offload-bundler, llvm-readelf, and c++filt.
"""
import argparse
import os
import re
import subprocess
import tempfile

BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
          ".sgpr_spill_count", ".kernarg_segment_size")


def _run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels(lib, arch="gfx950"):
    """{demangled kernel name: {field: int}}"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        _run(os.path.join(BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
        _run(os.path.join(BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch,
             "--input=" + fat, "--output=" + co)
        notes = _run(os.path.join(BIN, "llvm-readelf"), "--notes", co)
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^(?:  - |    )(\.[a-z_]+):\s*(.*)$", line)      # the fields of a kernel's record, not those of its arguments
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if line.startswith("  - "):
            cur = {}
        if cur is None:
            continue
        if key in FIELDS:
            cur[key] = int(val)
        elif key == ".name":
            out[val] = cur
    names = list(out)
    plain = _run("c++filt", *names).splitlines() if names else []
    return {p.split("(")[0].replace("void ", ""): out[n] for n, p in zip(names, plain)}


def instructions(lib, arch="gfx950"):
    """{demangled kernel name: md5 of its instruction text}: mnemonics and operands only, padding after the last instruction cut"""
    import hashlib
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        _run(os.path.join(BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
        _run(os.path.join(BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch,
             "--input=" + fat, "--output=" + co)
        dis = _run(os.path.join(BIN, "llvm-objdump"), "-d", co)
    out, name, buf = {}, None, []

    def close():
        if name is not None:
            while buf and buf[-1] in ("s_nop 0", "...", "s_code_end"):
                buf.pop()
            out[name] = hashlib.md5("\n".join(buf).encode()).hexdigest()
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            close()
            name, buf = m.group(1), []
        elif name is not None:
            t = re.sub(r"\s+", " ", line.split("//")[0].strip())
            if t:
                buf.append(t)
    close()
    names = list(out)
    plain = _run("c++filt", *names).splitlines() if names else []
    return {p.split("(")[0].replace("void ", ""): out[n] for n, p in zip(names, plain)}


def waves(r):
    v = r[".vgpr_count"]
    return min(8, 512 // max(8, (v + 7) // 8 * 8))


def row(r):
    return "%4d %4d %4d %7d %7d %5d %5d" % (r[".vgpr_count"], r.get(".agpr_count", 0), r[".sgpr_count"], r[".group_segment_fixed_size"],
                                            r[".private_segment_fixed_size"], r.get(".vgpr_spill_count", 0), waves(r))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib")
    ap.add_argument("--filter", default="", help="only kernels whose name contains this")
    ap.add_argument("--against", help="a second library to compare with (the older one)")
    ap.add_argument("--code", action="store_true", help="with --against: compare the instruction text of every kernel too")
    a = ap.parse_args()
    new = {k: v for k, v in kernels(a.lib).items() if a.filter in k}
    head = "vgpr agpr sgpr lds_B scratch_B spill waves"
    if not a.against:
        print("%-48s %s" % ("kernel", head))
        for k in sorted(new):
            print("%-48s %s" % (k, row(new[k])))
        return
    old = {k: v for k, v in kernels(a.against).items() if a.filter in k}
    print("%-48s %-8s %s   | %s" % ("kernel", "", head, head + "  (against)"))
    cmp_fields = [f for f in FIELDS if f != ".kernarg_segment_size"]
    code_new, code_old = (instructions(a.lib), instructions(a.against)) if a.code else ({}, {})
    identical = 0
    for k in sorted(set(new) | set(old)):
        if k not in old:
            print("%-48s %-8s %s" % (k, "new", row(new[k])))
        elif k not in new:
            print("%-48s %-8s %s   | %s" % (k, "gone", "", row(old[k])))
        else:
            same = all(new[k].get(f, 0) == old[k].get(f, 0) for f in cmp_fields)
            if a.code:
                same = same and code_new.get(k) is not None and code_new.get(k) == code_old.get(k)
                identical += same
            print("%-48s %-8s %s   | %s" % (k, "same" if same else "differs", row(new[k]), row(old[k])))
    if a.code:
        print("# %d of the %d kernels of the older library: same resources and the same instruction text in the newer one" % (identical, len(old)))


if __name__ == "__main__":
    main()
