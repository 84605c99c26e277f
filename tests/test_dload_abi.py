"""The distributed-load section of the C ABI (include/fistr_hip.h): declared, exported by the built library, and mirrored by the
ctypes structure of frontistr_amd/hecmw.py with the compiler's size and offsets.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fistr_hip.h")
NAMES = ("fx_dload_groups", "fx_dload_element", "fx_nl_set_dload", "fx_nl_set_dload_factor", "fx_nl_get_load", "fx_dload_get_stats")
MEMBERS = ("n", "group", "elem", "ltype", "params", "held")


def _args(text, name):
    return [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")]


def test_header_declares_and_library_exports(hip):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(fx_context \*ctx" % name, text), name
    assert re.search(r"\} fx_dload;", text)
    lib = hip.lib()
    for name in NAMES:
        assert getattr(lib, name) is not None
    assert _args(text, "fx_dload_groups") == ["ctx", "n_node", "coord", "n_group", "groups", "n_mat", "rho", "dl", "factor", "disp",
                                               "load_inout", "ms_kernel"]
    assert _args(text, "fx_dload_element") == ["ctx", "etype", "ltype", "ecoord", "rho", "params", "vect"]
    assert _args(text, "fx_nl_set_dload") == ["ctx", "n_mat", "rho", "dl", "follow"]
    assert _args(text, "fx_nl_set_dload_factor") == ["ctx", "factor"]
    assert _args(text, "fx_nl_get_load") == ["ctx", "GL"]
    assert _args(text, "fx_dload_get_stats") == ["ctx", "out[8]"]
    # the entry points the load reaches the solver through keep their argument lists
    assert _args(text, "fx_nl_begin_substep") == ["ctx", "GL"]
    assert _args(text, "fx_newton_substep") == ["ctx", "factor0", "factor1", "n_bc", "bc_node", "bc_dof", "bc_val", "cload", "max_iter",
                                                 "converg", "Iarray", "Rarray", "log", "n_iter", "commit_unconverged"]
    assert _args(text, "fx_assemble_groups") == ["ctx", "n_node", "coord", "n_group", "groups", "n_mat", "E", "nu", "load", "n_bc",
                                                  "bc_node", "bc_dof", "bc_val", "ms_assemble"]
    # what the sums are equal to from call to call is stated
    assert "not bit for bit" in text[text.index("typedef struct fx_dload"):]


def test_python_structure_matches_the_compiler(hip, tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], stdout=subprocess.DEVNULL).returncode == 0), None)
    if cc is None:
        pytest.fail("no C compiler to read the header with")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fistr_hip.h"', "int main(void) {",
             '  printf("%zu", sizeof(fx_dload));']
    lines += ['  printf(" %%zu", offsetof(fx_dload, %s));' % m for m in MEMBERS]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    size, *offs = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    T = hip._Dload
    assert C.sizeof(T) == int(size)
    assert tuple(f[0] for f in T._fields_) == MEMBERS
    assert [getattr(T, m).offset for m in MEMBERS] == [int(o) for o in offs]


def test_python_interface(hip):
    from frontistr_amd import fstr
    for name in ("dload_groups", "dload_element", "dload_stats"):
        assert callable(getattr(hip.SolverContext, name)), name
    p = inspect.signature(hip.SolverContext.dload_groups).parameters
    assert list(p)[1:] == ["coord", "groups", "rho", "dload", "factor", "disp", "load"]
    assert (p["factor"].default, p["disp"].default, p["load"].default) == (1.0, None, None)
    for name in ("body", "gravity", "centrifugal", "pressure"):
        assert callable(getattr(fstr.tDload, name)), name
    assert callable(fstr.dload_faces) and list(inspect.signature(fstr.dload_faces).parameters) == ["coord", "groups", "node_mask"]
    assert inspect.signature(fstr.fstr_solid.set_dload).parameters["follow"].default is True
    assert callable(fstr.fstr_solid.get_load)
    # the loop's drivers keep their signatures: the load factor reaches the list through fx_newton_substep
    assert list(inspect.signature(fstr.fstr_Newton).parameters) == ["fstrSOLID", "hecMAT", "factor", "bc", "cload", "max_iter", "converg",
                                                                     "commit_unconverged", "temperature", "time", "tincr"]
    assert list(inspect.signature(fstr.fstr_solve_NLGEOM).parameters) == ["fstrSOLID", "hecMAT", "bc", "cload", "substeps", "max_iter",
                                                                           "converg", "commit_unconverged", "temperature", "tincr",
                                                                           "start_time", "load_held"]


def test_null_arguments_are_refused_before_anything_is_touched(hip):
    lib = hip.lib()
    dl = hip._Dload()
    out = (C.c_int64 * 8)()
    assert lib.fx_dload_groups(None, 1, None, 1, None, 0, None, C.byref(dl), C.c_double(1.0), None, None, None) == -1
    assert b"null argument" in lib.fx_last_error()
    assert lib.fx_dload_element(None, 361, 1, None, C.c_double(0.0), None, None) == -1
    assert lib.fx_nl_set_dload(None, 0, None, C.byref(dl), 1) == -1
    assert lib.fx_nl_set_dload_factor(None, C.c_double(1.0)) == -1
    assert lib.fx_nl_get_load(None, None) == -1
    assert lib.fx_dload_get_stats(None, out) == -1
    assert b"null argument" in lib.fx_last_error()
