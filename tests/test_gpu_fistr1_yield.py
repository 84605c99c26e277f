"""fistr1 itself (oracle/_ref/fistr1_hip) with `!PLASTIC, YIELD=MOHR-COULOMB | DRUCKER-PRAGER` decks: with HECMW_GPU_NL_YIELD=1
fstr_StiffMatrix and fstr_UpdateNewton of every Newton iteration run on the device (material kinds 4 / 5 of fx_material_view, filled
from variables(M_PLCONST1:4)); without the switch the host loops run and nothing changes.  Decks: the reference's
examples/static/1elem/{drucker,mohr,mohrshear} and tutorial/06_plastic_can (committed copies under tests/golden/decks/), and one recorded cube
deck each of 342 and 362 with the type gate set as well.  They report the element loops on the device and reproduce the Newton
counts of FSTR.sta and the Global summaries of 0.log that the unmodified program recorded (tests/golden/yield_decks.npz; for the
tutorial the fixture the suite already holds) at the reference harness's 1e-4.

1elem/mohrshear (`!SOLUTION, TYPE = STATIC` with `!STATIC, TYPE = NLGEOM`, the older spelling of a nonlinear static analysis; it runs
on mohr.msh, see tests/yield_ref.py) is one of them."""
import json
import os
import sys

import numpy as np
import pytest

import yield_ref as Y
from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE = "### libfistr_hip: stiffness assembly and stress update on the device (TYPE="
YIELD = "### libfistr_hip: Mohr-Coulomb / Drucker-Prager materials on the device (HECMW_GPU_NL_YIELD=1)"


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_yield_golden as G
    return G


def _check(r, name, on_device):
    g = np.load(os.path.join(HERE, "golden", "yield_decks.npz"))
    want, newton = json.loads(str(g[name + "/log"])), [int(v) for v in g[name + "/newton"]]
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "reference CPU solver used" not in r["stdout"]
    out = r["stdout"]
    assert (DEVICE in out) == on_device and (YIELD in out) == on_device
    assert ("fstr_StiffMatrix on the device" in out) == on_device and ("fstr_UpdateNewton on the device" in out) == on_device
    assert [row[3] for row in r["sta"]] == newton, (r["sta"], newton)
    assert len(r["log"]) == len(want)
    for k, (a, c) in enumerate(zip(r["log"], want)):
        assert Y.within_1e4(a, c) == [], (k, Y.within_1e4(a, c))


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


@pytest.mark.parametrize("name", ["1elem_drucker", "1elem_mohr", "1elem_mohrshear"])
def test_reference_1elem_decks(name):
    _need()
    deck, mesh, cnt = _golden().REFERENCE_DECKS[name]
    r = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_NL_YIELD": "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, True)
    # the same deck without the switch: the host loops, the same recorded numbers
    host = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
    _check(host, name, False)


def test_tutorial_06_plastic_can_on_the_device():
    """tutorial/06_plastic_can (Drucker-Prager, TYPE=342, 7236 elements, 10 sub-steps) with both gates: the element loops are
    reported on the device, Newton counts [2] * 10 and every step's extrema as the fixture the suite holds (the unmodified
    program's 0.log)."""
    _need()
    r = f1.run_deck("fistr1_hip", "t06", "can.msh", "can.cnt",
                    env={"HECMW_GPU_NL_TET": "1", "HECMW_GPU_NL_YIELD": "1", "HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    out = r["stdout"]
    assert DEVICE + "342)" in out and YIELD in out
    assert "fstr_StiffMatrix on the device" in out and "fstr_UpdateNewton on the device" in out
    assert [x[3] for x in r["sta"]] == [2] * 10, r["sta"]
    want = f1.read_log(os.path.join(f1.DECKS, "t06", "can_fistr1_ref_0.log"))
    assert len(r["log"]) == len(want) == 11
    for k, (a, c) in enumerate(zip(r["log"], want)):
        assert f1.compare_step(a, c) == [], k
    _check(r, "t06_can", True)


@pytest.mark.parametrize("name,gate", [("y342_mohr_two", "HECMW_GPU_NL_TET"), ("y362_drucker", "HECMW_GPU_NL_C3")])
def test_recorded_cube_decks(name, gate, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_NL_YIELD": "1", gate: "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, True)
    # the type's own gate still applies
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_NL_YIELD": "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, False)
