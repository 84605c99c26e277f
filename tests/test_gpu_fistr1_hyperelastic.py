"""fistr1 itself (oracle/_ref/fistr1_hip) with `!HYPERELASTIC` decks: with HECMW_GPU_NL_HYPER=1 fstr_StiffMatrix and fstr_UpdateNewton
of every Newton iteration run on the device (material kinds 2 / 3 of fx_material_view, filled from variables(M_PLCONST1:3)); without
the switch the host loops run.  Decks: the reference's examples/static/1elem/{rivlin,arruda} and tutorial/03_hyperelastic_cylinder
(committed copies under tests/golden/decks/), and one recorded cube deck each of 342 and 362 with the type gate set as well.  They
report the element loops on the device and reproduce the Newton counts of FSTR.sta and the Global summaries of 0.log that the
unmodified program recorded (tests/golden/hyper_decks.npz) at the reference harness's 1e-4, the difference of the printed decimals
taken exactly (hyper_ref.within_1e4).

1elem/arruda (D = 1.429e-8, bulk term 1 / D = 7e7): the lateral stress S22 = S33 of step 4 is the remainder Newton leaves at the
displacement criterion, 6.75745 to within 2e-8, on the rounding edge of the five digits the log prints.  The unmodified program's own
log prints 6.7575 for S22 and 6.7574 for S33 of its one element; the device run prints 6.7574 for both.  Either digit is within the
bound of the other, which the float subtraction 6.7575 - 6.7574 = 1.0000000000065512e-4 does not see;
tests/test_hyper_1elem_ref.py asserts the evidence.  The test below also runs this deck with the host loops (same binary, same
device Krylov solver, no HECMW_GPU_NL_HYPER) -- the reference's own element code -- and holds both runs to the recorded log and to each
other at the same bound.

1elem/neohooke is not run: the unmodified program does not converge on it (NaN residual from the first Newton iteration, stop at the
50th), recorded in tests/golden/hyper_1elem_neohooke.json and asserted in tests/test_hyper_1elem_ref.py; there is no FSTR.sta count
and no summary to reproduce, and a run that fills the device solver with NaN for 50 iterations of 10000 is not a test."""
import json
import os
import sys

import numpy as np
import pytest

import hyper_ref as H
from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE = "### libfistr_hip: stiffness assembly and stress update on the device (TYPE="
HYPER = "### libfistr_hip: hyperelastic materials on the device (HECMW_GPU_NL_HYPER=1)"


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_hyper_golden as G
    return G


def _check(r, name, on_device):
    g = np.load(os.path.join(HERE, "golden", "hyper_decks.npz"))
    want, newton = json.loads(str(g[name + "/log"])), [int(v) for v in g[name + "/newton"]]
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "reference CPU solver used" not in r["stdout"]
    out = r["stdout"]
    assert (DEVICE in out) == on_device and (HYPER in out) == on_device
    assert ("fstr_StiffMatrix on the device" in out) == on_device and ("fstr_UpdateNewton on the device" in out) == on_device
    assert [row[3] for row in r["sta"]] == newton, (r["sta"], newton)
    assert len(r["log"]) == len(want)
    for k, (a, c) in enumerate(zip(r["log"], want)):
        assert H.within_1e4(a, c) == [], k


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


@pytest.mark.parametrize("name", ["1elem_rivlin", "1elem_arruda", "t03_cylinder"])
def test_reference_decks_on_the_device(name):
    _need()
    deck, mesh, cnt = _golden().REFERENCE_DECKS[name]
    r = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_NL_HYPER": "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, True)
    if name == "1elem_arruda":
        host = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
        _check(host, name, False)
        for k, (a, c) in enumerate(zip(r["log"], host["log"])):
            assert H.within_1e4(a, c) == [], k
        print("step 4, device loops:", r["log"][4]["Element"]["S22"], r["log"][4]["Element"]["S33"], "host loops:",
              host["log"][4]["Element"]["S22"], host["log"][4]["Element"]["S33"])


@pytest.mark.parametrize("name,gate", [("h342_arruda_two", "HECMW_GPU_NL_TET"), ("h362_mooney", "HECMW_GPU_NL_C3")])
def test_recorded_cube_decks(name, gate, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_NL_HYPER": "1", gate: "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, True)
    # the type's own gate still applies
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_NL_HYPER": "1", "HECMW_GPU_REPORT": "1"})
    _check(r, name, False)


def test_without_the_switch_the_host_loops_run():
    _need()
    deck, mesh, cnt = _golden().REFERENCE_DECKS["1elem_rivlin"]
    r = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
    _check(r, "1elem_rivlin", False)
