"""fistr1 itself on NLSTATIC decks with a `!TEMPERATURE` load on the device: oracle/_ref/fistr1_hip with HECMW_GPU_NL_THERMAL=1 (plus
the type's own opt-in) runs fstr_StiffMatrix and fstr_UpdateNewton through the thermal variants of the nonlinear element kernels
(fx_nl_set_thermal filled from M_EXAPNSION, MC_THEMOEXP, MC_ISOELASTIC, ref_temp and the initial condition; fstrSOLID%temperature
uploaded before every call; the thermal load stays in the reference's fstr_ass_load).  Decks: the recorded cube decks of
tests/golden/make_nl_thermal_golden.py at 361 and 341 / 342 (Mises updated Lagrange with an initial condition, constants, tables) and
the reference's own examples/static/thermal_stress/sample1 (`!TEMPERATURE, READRESULT=8`).  The report line ends in `, thermal`, the
Newton count of every sub-step is the one recorded from the unmodified program (tests/golden/nl_thermal_decks.npz) and the last
step's summary matches it at the reference harness's 1e-4.  A deck with orthotropic expansion, or with a temperature column in
`!PLASTIC`, keeps the host loops.

Must fail without the feature: before it every such deck printed `fstr_StiffMatrix on the host`."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENV = {"HECMW_GPU_NL_THERMAL": "1", "HECMW_GPU_NL_C3": "1", "HECMW_GPU_REPORT": "1"}
DEVICE = ("fstr_StiffMatrix on the device", "fstr_UpdateNewton on the device", "keeps them on the host, thermal")


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_nl_thermal_golden as G
    return G


def _record(name):
    g = np.load(os.path.join(HERE, "golden", "nl_thermal_decks.npz"))
    return json.loads(str(g[name + "/log"])), [int(x) for x in g[name + "/newton"]]


def _check(r, name):
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    for line in DEVICE:
        assert line in r["stdout"], line
    assert "fstr_StiffMatrix on the host" not in r["stdout"]
    rlog, newton = _record(name)
    print(name, "Newton iterations per sub-step", [row[3] for row in r["sta"]], "recorded", newton)
    assert [row[3] for row in r["sta"]] == newton
    assert f1.compare_step(r["log"][-1], rlog[-1]) == []


@pytest.mark.parametrize("name", ["t361_mises_ic", "t361_elastic_tab", "t341_elastic", "t342_elastic_tab"])
def test_recorded_cube_decks_on_the_device(name, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    _check(f1.run("fistr1_hip", d, env=ENV), name)


def test_thermal_stress_sample1_on_the_device(tmp_path):
    _need()
    d = str(tmp_path / "deck")
    os.makedirs(d)
    _check(_golden().run_sample1(d, "fistr1_hip", ENV), "thermal_stress1")


def _edited(tmp_path, name, old, new):
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    assert s.count(old) == 1
    with open(p, "w") as fh:
        fh.write(s.replace(old, new))
    return d


@pytest.mark.parametrize("case", ["orthotropic", "yield_temperature"])
def test_decks_outside_the_thermal_scope_keep_the_host_loops(case, tmp_path):
    """Orthotropic expansion (MC_ORTHOEXP) and a temperature column in the yield table are not on the device: with every switch set
    the gate keeps the host element loops and the run completes"""
    _need()
    if case == "orthotropic":
        d = _edited(tmp_path, "t341_elastic", "!EXPANSION_COEFF\n 1.2e-05\n", "!EXPANSION_COEFF, TYPE=ORTHOTROPIC\n 1.2e-05, 1.2e-05, 1.2e-05\n")
    else:
        rows = "".join(" %s, %s, %s\n" % (y * f, p, t) for t, f in ((0.0, 1.0), (500.0, 0.9))
                       for y, p in ((450.0, 0.0), (608.0, 0.05), (679.0, 0.1), (732.0, 0.2), (752.0, 0.3), (766.0, 0.4), (780.0, 0.5)))
        old = ("!PLASTIC, YIELD=MISES, HARDEN=MULTILINEAR\n 450.0, 0.0\n 608.0, 0.05\n 679.0, 0.1\n 732.0, 0.2\n 752.0, 0.3\n 766.0, 0.4\n"
               " 780.0, 0.5\n")
        d = _edited(tmp_path, "t361_mises_ic", old, "!PLASTIC, YIELD=MISES, HARDEN=MULTILINEAR, DEPENDENCIES=1\n" + rows)
    r = f1.run("fistr1_hip", d, env=ENV)
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    for line in DEVICE:
        assert line not in r["stdout"], line
    assert "fstr_StiffMatrix on the host" in r["stdout"] and len(r["sta"]) == 3
