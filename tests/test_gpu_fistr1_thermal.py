"""fistr1 itself with the reference's thermal-stress decks (examples/static/exF, all six solid types) on the device:
oracle/_ref/fistr1_hip with HECMW_GPU_THERMAL=1 (thermal decks opt in: DESIGN.md section 7) and HECMW_GPU_UPDATE=1 runs
fstr_StiffMatrix through the assembly kernels and fstr_UpdateNewton through fx_update_groups_linear_thermal; the thermal load
vector stays in the reference's fstr_ass_load on the host.  Each run reports both on the device, the report line
ends in `, thermal`, and the result matches the deck's `_correct.log` at the reference harness's 1e-4, as the static-suite test
asks.  Without the switch the same decks keep the host loops
(test_gpu_fistr1_c3.py, test_gpu_fistr1_tet.py).  NLGEOM decks with a `!TEMPERATURE` load keep the host loops with the switch
set: the cube decks of scripts/fistr1_cube_deck.py (TYPE=361 B-bar, which runs on the device by default, and TYPE=341 with its
own opt-in set) edited the way test_gpu_fistr1_tet_nonlinear.py edits its thermal deck.

Must fail without the feature: before it no thermal deck printed `stiffness assembly on the device`."""
import os
import subprocess
import sys

import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
ENV = {"HECMW_GPU_REPORT": "1", "HECMW_GPU_THERMAL": "1", "HECMW_GPU_UPDATE": "1"}


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (build() makes it where the reference sources are present)")


@pytest.mark.parametrize("etype", [341, 342, 351, 352, 361, 362])
def test_exF_on_the_device(etype):
    _need()
    model = "F%d" % etype
    r = f1.run_deck("fistr1_hip", os.path.join("static", "exF"), model + ".msh", "F300.cnt", env=ENV)
    out = r["stdout"]
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in out, out[-2000:]
    assert "reference CPU solver used" not in out
    line = "### libfistr_hip: stiffness assembly on the device (linear static, TYPE=%d); HECMW_GPU_ASSEMBLY=0 keeps it on the host, thermal" % etype
    assert line in out
    assert "fstr_StiffMatrix on the device" in out and "fstr_UpdateNewton on the device" in out
    correct = f1.read_log(os.path.join(f1.DECKS, "static", "exF", model + "_correct.log"))
    assert correct and f1.compare_step(r["log"][-1], correct[-1]) == []


@pytest.mark.parametrize("args", [["2", "2", "--etype", "341", "--nl-material", "elastic_tl"], ["2", "2"]], ids=["341", "361"])
def test_nlgeom_thermal_deck_keeps_the_host_loops(args, tmp_path):
    """An NLSTATIC cube deck with an expansion coefficient and 10 degrees on the top face, every switch that could move it to the
    device set (HECMW_GPU_THERMAL, HECMW_GPU_UPDATE, HECMW_GPU_NL_C3): the nonlinear gate keeps the host loops, no report line
    puts an element loop on the device, the run completes and matches the unmodified program where it is built."""
    _need()
    d = str(tmp_path / "deck")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, "scripts", "fistr1_cube_deck.py"), d] + args, check=True, stdout=subprocess.DEVNULL)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    step, elastic = "!STEP, SUBSTEPS=2, CONVERG=1.0e-3\n BOUNDARY, 1\n", "!ELASTIC\n 206900.0, 0.29\n"
    assert step in s and elastic in s
    s = s.replace(step, "!TEMPERATURE\n TOP, 10.0\n!REFTEMP\n 0.0\n" + step).replace(elastic, elastic + "!EXPANSION_COEFF\n 1.0e-5\n")
    with open(p, "w") as fh:
        fh.write(s)
    r = f1.run("fistr1_hip", d, env=dict(ENV, HECMW_GPU_NL_C3="1"))
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    for line in ("stiffness assembly", "fstr_StiffMatrix on the device", "fstr_UpdateNewton on the device"):
        assert line not in r["stdout"], line          # (the solve itself stays on the device: `solved on the device`)
    assert "fstr_StiffMatrix on the host" in r["stdout"] and len(r["sta"]) == 2
    if f1.have("fistr1_ref"):
        ref = f1.run("fistr1_ref", d, threads=2)
        assert f1.compare_step(r["log"][-1], ref["log"][-1]) == []
