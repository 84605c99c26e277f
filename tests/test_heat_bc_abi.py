"""The surface-term section of the C ABI (include/fistr_hip.h): declared, exported by the built library, and mirrored by the
ctypes structures of frontistr_amd/hecmw.py with the compiler's sizes and offsets.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fistr_hip.h")
NAMES = ("fx_heat_assemble_groups_bc", "fx_heat_face", "fx_heat_get_bc_stats")
STRUCTS = {"fx_heat_surface": ("n", "group", "elem", "face", "val", "sink"), "fx_heat_bc": ("dflux", "film", "radiate", "tzero")}


def _args(text, name):
    return [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")]


def test_header_declares_and_library_exports(hip):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(fx_context \*ctx" % name, text), name
    for s in STRUCTS:
        assert re.search(r"\} %s;" % s, text), s
    lib = hip.lib()
    for name in NAMES + ("fx_heat_assemble_groups", "fx_heat_get_stats"):
        assert getattr(lib, name) is not None
    # the arguments of fx_heat_assemble_groups up to fix_val, then bc and ms_kernel; the old entry point keeps its signature
    old = _args(text, "fx_heat_assemble_groups")
    assert old == ["ctx", "n_node", "coord", "n_group", "groups", "n_mat", "mats", "heat", "mat", "flux", "n_fix", "fix_node", "fix_val", "ms_kernel"]
    assert _args(text, "fx_heat_assemble_groups_bc") == old[:-1] + ["bc", "ms_kernel"]
    assert _args(text, "fx_heat_face") == ["ctx", "etype", "kind", "face", "ecoord", "tt", "val", "sink", "tzero", "term1", "term2", "nsuf", "mm"]
    assert "reorders only a sum into B" in text          # the position of !CFLUX is stated


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
    mirror = {"fx_heat_surface": hip._HeatSurface, "fx_heat_bc": hip._HeatBc}
    seen = 0
    for line in filter(None, out):
        name, size, *offs = line.split()
        T = mirror[name]
        assert C.sizeof(T) == int(size), name
        assert [getattr(T, m).offset for m in STRUCTS[name]] == [int(o) for o in offs], name
        assert tuple(f[0] for f in T._fields_) == STRUCTS[name]
        seen += 1
    assert seen == 2


def test_python_interface(hip):
    from frontistr_amd import heat
    for name in ("heat_assemble_groups", "heat_face", "heat_bc_stats"):
        assert callable(getattr(hip.SolverContext, name))
    for name in ("tHeatAmplitude", "heat_get_amplitude", "surface_of_egroup", "heat_solve_SS", "heat_solve_TRAN"):
        assert callable(getattr(heat, name))
    p = inspect.signature(hip.SolverContext.heat_assemble_groups).parameters
    assert all(p[k].default is None for k in ("dflux", "film", "radiate")) and p["tzero"].default == 0.0
    for f in (heat.heat_solve_SS, heat.heat_solve_TRAN):
        p = inspect.signature(f).parameters
        assert all(p[k].default is None for k in ("dflux", "film", "radiate", "fix_amplitude", "flux_amplitude")) and p["tzero"].default == 0.0
