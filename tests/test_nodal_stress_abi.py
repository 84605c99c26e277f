"""The nodal stress section of the C ABI (include/fistr_hip.h): declared, exported by the built library, and mirrored by the
ctypes structure of frontistr_amd/hecmw.py with the compiler's sizes and offsets.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fistr_hip.h")
NAMES = ("fx_nodal_stress_groups", "fx_nl_nodal_stress", "fx_nodal_get_stats")
MEMBERS = ("n_node", "n_elem", "strain", "stress", "mises", "estrain", "estress", "emises", "pstress", "pstress_vect", "pstrain",
           "pstrain_vect", "epstress", "epstress_vect", "epstrain", "epstrain_vect")


def _args(text, name):
    return [a.strip().split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1).split(",")]


def test_header_declares_and_library_exports(hip):
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(fx_context \*ctx" % name, text), name
    assert re.search(r"\} fx_nodal_result;", text)
    lib = hip.lib()
    for name in NAMES + ("fx_nodal_inverse", "fx_update_groups_linear", "fx_nl_get_state"):
        assert getattr(lib, name) is not None
    assert _args(text, "fx_nodal_stress_groups") == ["ctx", "n_node", "n_group", "groups", "strain", "stress", "flags", "out", "ms_kernel"]
    assert _args(text, "fx_nl_nodal_stress") == ["ctx", "flags", "out", "ms_kernel"]
    # the entry points this one is fed from keep their argument lists
    assert _args(text, "fx_update_groups_linear") == ["ctx", "n_node", "coord", "n_group", "groups", "n_mat", "E", "nu", "disp", "strain",
                                                       "stress", "qforce", "ms_kernel"]
    # the index order of the vector arrays and the life time of the pointers are stated
    assert "vect[(i * 3 + j) * 3 + r]" in text and "valid until the next nodal-stress call" in text
    # the flag bits are make_principal's
    bits = dict(re.findall(r"(FX_PRINCV?_[NE]STR(?:ESS|AIN)) = (\d+)", text))
    assert {k: int(v) for k, v in bits.items()} == {"FX_PRINC_NSTRESS": 1, "FX_PRINCV_NSTRESS": 2, "FX_PRINC_NSTRAIN": 4, "FX_PRINCV_NSTRAIN": 8,
                                                    "FX_PRINC_ESTRESS": 16, "FX_PRINCV_ESTRESS": 32, "FX_PRINC_ESTRAIN": 64,
                                                    "FX_PRINCV_ESTRAIN": 128}
    assert (hip.PRINC_NSTRESS, hip.PRINCV_NSTRESS, hip.PRINC_NSTRAIN, hip.PRINCV_NSTRAIN, hip.PRINC_ESTRESS, hip.PRINCV_ESTRESS,
            hip.PRINC_ESTRAIN, hip.PRINCV_ESTRAIN) == (1, 2, 4, 8, 16, 32, 64, 128)


def test_python_structure_matches_the_compiler(hip, tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["which", c], stdout=subprocess.DEVNULL).returncode == 0), None)
    if cc is None:
        pytest.fail("no C compiler to read the header with")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fistr_hip.h"', "int main(void) {",
             '  printf("%zu", sizeof(fx_nodal_result));']
    lines += ['  printf(" %%zu", offsetof(fx_nodal_result, %s));' % m for m in MEMBERS]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    size, *offs = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    T = hip._NodalResult
    assert C.sizeof(T) == int(size)
    assert tuple(f[0] for f in T._fields_) == MEMBERS
    assert [getattr(T, m).offset for m in MEMBERS] == [int(o) for o in offs]


def test_python_interface(hip):
    from frontistr_amd import fstr
    assert callable(hip.SolverContext.nodal_stress_groups) and callable(hip.SolverContext.nodal_stats)
    assert callable(fstr.fstr_solid.nodal_stress) and callable(fstr.fstr_NodalStress3D)
    assert inspect.signature(hip.SolverContext.nodal_stress_groups).parameters["principal"].default == 0
    assert inspect.signature(fstr.fstr_solid.nodal_stress).parameters["principal"].default == 0
    assert callable(hip.NodalStress.summary)


def test_null_arguments_are_refused_before_anything_is_touched(hip):
    lib = hip.lib()
    res = hip._NodalResult()
    assert lib.fx_nl_nodal_stress(None, 0, C.byref(res), None) == -1
    assert lib.fx_nodal_stress_groups(None, 1, 0, None, None, None, 0, C.byref(res), None) == -1
    assert b"null argument" in lib.fx_last_error()


def test_the_inverses_are_inverse_func_s(hip):
    """The constants the kernels take are made on the host (no device needed): bit for bit those of the numpy restatement of
    inverse_func, and not those of a library inverse."""
    import nodal_stress_ref as NR
    lib = hip.lib()
    differs = 0
    for etype, n in ((361, 8), (342, 4), (352, 6), (362, 8)):
        inv, got_n = np.zeros((n, n)), C.c_int32(0)
        assert lib.fx_nodal_inverse(etype, inv.ctypes.data_as(C.c_void_p), C.byref(got_n)) == 0 and got_n.value == n
        assert np.array_equal(inv, NR.inverse(etype)), etype
        func = np.array([NR.vertex_shape(etype, NR.quad_point(etype, q)) for q in NR.SEL[etype]])
        assert np.abs(inv @ func - np.eye(n)).max() < 1e-13
        differs += int(not np.array_equal(inv, np.linalg.inv(func)))
    assert differs > 0
    got_n = C.c_int32(-1)
    assert lib.fx_nodal_inverse(341, None, C.byref(got_n)) == 0 and got_n.value == 0
    assert lib.fx_nodal_inverse(301, None, C.byref(got_n)) == -2
