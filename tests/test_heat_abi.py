"""The heat section of the C ABI (include/fistr_hip.h): declared, exported by the built library, and mirrored by the ctypes
structures of frontistr_amd/hecmw.py with the compiler's sizes and offsets.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fistr_hip.h")
NAMES = ("fx_heat_assemble_groups", "fx_heat_element", "fx_heat_get_stats")
STRUCTS = {"fx_heat_table": ("ntab", "temp", "funcA", "funcB"), "fx_heat_material_view": ("cond", "cp", "rho"),
           "fx_heat_view": ("temp", "temp0", "beta", "dtime")}


def test_header_declares_and_library_exports(hip):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(fx_context \*ctx" % name, text), name
    for s in STRUCTS:
        assert re.search(r"\} %s;" % s, text), s
    lib = hip.lib()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert "fx_heat_assemble_groups(ctx, n_node, coord, n_group, groups, n_mat, mats, heat, mat, flux, n_fix, fix_node, fix_val, ms_kernel)" == \
        "fx_heat_assemble_groups(" + ", ".join(
            a.strip().split()[-1].lstrip("*") for a in re.search(r"int fx_heat_assemble_groups\((.*?)\);", text, re.S).group(1).split(",")) + ")"


def test_python_structures_match_the_compiler(hip, tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], stdout=subprocess.DEVNULL).returncode == 0), None)
    if cc is None:
        pytest.fail("no C compiler to read the header with")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fistr_hip.h"', "int main(void) {"]
    for s, members in STRUCTS.items():
        lines.append('  printf("%s %%zu", sizeof(%s));' % (s, s))
        for m in members:
            lines.append('  printf(" %%zu", offsetof(%s, %s));' % (s, m))
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split("\n")
    mirror = {"fx_heat_table": hip._HeatTable, "fx_heat_material_view": hip._HeatMaterialView, "fx_heat_view": hip._HeatView}
    for line in filter(None, out):
        name, size, *offs = line.split()
        T = mirror[name]
        assert C.sizeof(T) == int(size), name
        assert [getattr(T, m).offset for m in STRUCTS[name]] == [int(o) for o in offs], name
        assert tuple(f[0] for f in T._fields_) == STRUCTS[name]


def test_python_interface(hip):
    from frontistr_amd import heat
    for name in ("heat_assemble_groups", "heat_element", "heat_stats"):
        assert callable(getattr(hip.SolverContext, name))
    for name in ("tHeatMaterial", "heat_solve_SS", "heat_solve_TRAN", "heat_matrix"):
        assert callable(getattr(heat, name))
    assert sys.modules["frontistr_amd.heat"].hecmw is hip
