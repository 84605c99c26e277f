"""fistr1 itself with decks of SEVERAL solid element types on the device (oracle/_ref/fistr1_hip, the reference's main program
with the binding of frontistr_amd/shim/): a linear static mesh whose types are all among 361, 341, 342, 351, 352, 362 runs
fstr_StiffMatrix through fx_assemble_groups, one group per entry of hecMESH%elem_type_item; fstr_UpdateNewton runs through
fx_update_groups_linear with HECMW_GPU_UPDATE=1 (opt-in for a mixed mesh: DESIGN.md section 4).

Must fail without the feature: no run of a mixed mesh printed
`### libfistr_hip: stiffness assembly on the device (linear static, TYPE=341+351+361)`; the element loops stayed on the host.

The reference's refine/hexpritet (361 + 351 + 341) and refine/tetpri (341 + 351) decks, unrefined, and the cube decks of
scripts/fistr1_cube_deck.py --mixed 1|2: the report line names the types in hecMESH's order (ascending), device against HECMW_GPU_ASSEMBLY=0 at
1e-7 (the bound of test_gpu_fistr1_c3.py) and against the unmodified program's extrema recorded in tests/golden/mixed_decks.npz
(make_mixed_golden.py) at the regression harness' 1e-4.  A mesh holding a type outside the six (one 301 truss beside the
solids) completes with the host loops and without the device line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _line(types):
    """The types in the order of hecMESH%elem_type_item: HEC-MW's reader sorts the element types ascending, whatever the order of
    the !ELEMENT cards, so a 361 + 351 + 341 file reports TYPE=341+351+361."""
    types = sorted(types)
    return ("### libfistr_hip: stiffness assembly on the device (linear static, TYPE=%s); HECMW_GPU_ASSEMBLY=0 keeps it on the host"
            % "+".join(str(t) for t in types))


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (build() makes it where the reference sources are present)")


def _modes(run):
    out = {}
    for mode, env in (("device", {}), ("update", {"HECMW_GPU_UPDATE": "1"}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


def _check(runs, types, ref):
    dev, upd, host = runs["device"]["stdout"], runs["update"]["stdout"], runs["host"]["stdout"]
    assert _line(types) in dev and "fstr_StiffMatrix on the device" in dev and "fstr_UpdateNewton on the host" in dev
    assert _line(types) in upd and "fstr_StiffMatrix on the device" in upd and "fstr_UpdateNewton on the device" in upd
    assert "stiffness assembly on the device" not in host and "fstr_StiffMatrix on the host" in host
    b = runs["host"]["log"][-1]
    for mode in ("device", "update"):
        a = runs[mode]["log"][-1]
        assert len(a["Node"]) >= 10 and f1.compare_step(a, b, threshold=1e-7) == [], mode
        assert f1.compare_step(a, ref) == [], mode


def _recorded(name):
    g = np.load(os.path.join(HERE, "golden", "mixed_decks.npz"))
    return json.loads(str(g[name + "/log"]))


@pytest.mark.parametrize("name,types", [("hexpritet", (361, 351, 341)), ("tetpri", (341, 351))])
def test_reference_mixed_decks_assemble_on_the_device(name, types):
    _need()
    runs = _modes(lambda env: f1.run_deck("fistr1_hip", os.path.join("refine", name), "sample.msh", "sample.cnt", env=env, iterlog="NO"))
    _check(runs, types, _recorded(name))


CUBES = [("m1_n2", 1, 2, False), ("m1_n2_two", 1, 2, True), ("m2_n2", 2, 2, False), ("m2_n2_two", 2, 2, True)]


@pytest.mark.parametrize("name,order,n,two", CUBES, ids=[c[0] for c in CUBES])
def test_mixed_cube_decks(name, order, n, two, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, str(n), "--linear", "--mixed", str(order)]
    subprocess.run(cmd + (["--two-sections"] if two else []), check=True, stdout=subprocess.DEVNULL)
    runs = _modes(lambda env: f1.run("fistr1_hip", d, env=env))
    _check(runs, (361, 351, 341) if order == 1 else (362, 352, 342), _recorded(name))


def test_a_type_outside_the_six_keeps_the_host_loops(tmp_path):
    """The --mixed 1 cube with one TYPE=301 truss added along an edge of the first hexahedron (the 371 pyramids of the
    reference's refine/hexpyr stop this build of the program itself: "element type not defined"): fistr1 must complete on the
    host loops."""
    _need()
    d = str(tmp_path / "deck")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, "2", "--linear", "--mixed", "1"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    msh = os.path.join(d, "cube.msh")
    s = open(msh).read()
    assert "!MATERIAL,NAME=MAT1" in s
    open(msh, "w").write(s.replace("!MATERIAL,NAME=MAT1", "!ELEMENT,TYPE=301,EGRP=E1\n23,1,2\n!MATERIAL,NAME=MAT1", 1))
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    assert "fstr_StiffMatrix on the host" in r["stdout"]
