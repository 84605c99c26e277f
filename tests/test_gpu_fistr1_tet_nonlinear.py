"""fistr1 itself (oracle/_ref/fistr1_hip) with nonlinear tetrahedral decks: `!STATIC, TYPE=NLGEOM` meshes of TYPE=341 or 342 only
run fstr_StiffMatrix and fstr_UpdateNewton of every Newton iteration on the device (fx_nl_init_c3) when HECMW_GPU_NL_TET=1 asks
for it (the tetrahedra opt in; without the switch the host loops run).  The reference's exI decks
A341 / A342 under I300.cnt (10 sub-steps, total Lagrange) print the device line, match their *_correct.log at the reference
harness's 1e-4 in every step and the same program with HECMW_GPU_ASSEMBLY=0 at 1e-7, with equal Newton counts per sub-step; the
recorded cube decks (tests/golden/nl_tet_decks.npz) match the host loops at 1e-7, the unmodified program's run at 1e-4 and its
Newton counts; a thermal tet deck keeps the host loops."""
import os
import subprocess
import sys

import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _line(etype):
    return ("### libfistr_hip: stiffness assembly and stress update on the device (TYPE=%d); HECMW_GPU_ASSEMBLY=0 keeps them on the host"
            % etype)


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _both(run):
    out = {}
    for mode, env in (("device", {"HECMW_GPU_NL_TET": "1"}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


@pytest.mark.parametrize("etype", [341, 342])
def test_exI_tetrahedra_on_the_device(etype):
    _need()
    model = "A%d" % etype
    runs = _both(lambda env: f1.run_deck("fistr1_hip", "exI", model + ".msh", "I300.cnt", env=env))
    dev, host = runs["device"]["stdout"], runs["host"]["stdout"]
    assert _line(etype) in dev and "fstr_StiffMatrix on the device" in dev and "fstr_UpdateNewton on the device" in dev
    assert "on the device (TYPE=" not in host and "fstr_StiffMatrix on the device" not in host and "fstr_UpdateNewton on the device" not in host
    correct = f1.read_log(os.path.join(f1.DECKS, "exI", model + "_correct.log"))
    a, b = runs["device"]["log"][1:], runs["host"]["log"][1:]      # 0.log opens with the summary of the initial state
    assert len(correct) == 10 and len(a) == 10 and len(b) == 10
    for k in range(10):
        assert f1.compare_step(a[k], correct[k]) == [], k
        assert f1.compare_step(a[k], b[k], threshold=1e-7) == [], k
    assert runs["device"]["sta"] == runs["host"]["sta"] and len(runs["device"]["sta"]) == 10


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_nl_tet_golden as G
    return G


@pytest.mark.parametrize("name", ["t341_elastic_tl", "t341_elastic_ul", "t341_bilinear", "t341_multilinear_two",
                                  "t342_elastic_tl", "t342_elastic_ul", "t342_bilinear", "t342_multilinear_two"])
def test_recorded_cube_decks(name, tmp_path):
    """The recorded cube decks (tests/golden/make_nl_tet_golden.py writes them with scripts/fistr1_cube_deck.py): the device run
    against the host loops at 1e-7, against the unmodified program's summaries in nl_tet_decks.npz at 1e-4, and the FSTR.sta rows
    with the Newton count of every sub-step equal in all three."""
    import json
    import numpy as np
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck(name, d)
    etype = G.DECKS[name][0]
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    assert _line(etype) in runs["device"]["stdout"] and "fstr_UpdateNewton on the device" in runs["device"]["stdout"]
    assert "on the device (TYPE=" not in runs["host"]["stdout"]
    a, b = runs["device"]["log"], runs["host"]["log"]
    g = np.load(os.path.join(HERE, "golden", "nl_tet_decks.npz"))
    want = json.loads(str(g[name + "/log"]))
    assert len(a) == len(b) == len(want) >= 3
    for k, (x, y, z) in enumerate(zip(a, b, want)):
        bad = f1.compare_step(x, y, threshold=1e-7)
        print(name, "step", k, "device against host at 1e-7:", bad)
        assert bad == [], k
        assert f1.compare_step(x, z) == [], k
    assert runs["device"]["sta"] == runs["host"]["sta"]
    assert [row[3] for row in runs["device"]["sta"]] == [int(v) for v in g[name + "/newton"]]


def test_thermal_tet_deck_keeps_the_host_loops(tmp_path):
    """An NLGEOM tet deck with a `!TEMPERATURE` load (the elastic total-Lagrange 341 cube with an expansion coefficient and 10
    degrees on the top face): the nonlinear gate's thermal test keeps the host loops, no device-assembly line, the run completes
    and matches the unmodified program where it is built."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("t341_elastic_tl", d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    step, elastic = "!STEP, SUBSTEPS=3, CONVERG=1.0e-3\n BOUNDARY, 1\n", "!ELASTIC\n 206900.0, 0.29\n"
    assert step in s and elastic in s
    s = s.replace(step, "!TEMPERATURE\n TOP, 10.0\n!REFTEMP\n 0.0\n" + step).replace(elastic, elastic + "!EXPANSION_COEFF\n 1.0e-5\n")
    with open(p, "w") as fh:
        fh.write(s)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    assert "fstr_StiffMatrix on the host" in r["stdout"] and len(r["sta"]) == 3
    if f1.have("fistr1_ref"):
        ref = f1.run("fistr1_ref", d, threads=2)
        assert f1.compare_step(r["log"][-1], ref["log"][-1]) == []


AUTOINC = ("!AUTOINC_PARAM, NAME=AP1\n 0.25, 10, 50, 10, 1\n 1.25, 10, 1, 2, 2\n 0.5, 8\n"
           "!STEP, SUBSTEPS=40, CONVERG=1.0e-3, MAXITER=10, INC_TYPE=AUTO, AUTOINCPARAM=AP1\n 0.34, 1.0, 1.0e-6, 0.34\n BOUNDARY, 1\n")


def test_automatic_incrementation_with_cutback(tmp_path):
    """The Mises BILINEAR 341 cube with `!AUTOINC_PARAM` and MAXITER=10: Newton runs into MAXITER, the state is rolled back
    (fstr_cutback_load -> fx_nl_snapshot) and the increment cut, at least once.  The sub-step sequence of FSTR.sta (status, Newton
    iterations) is the same on the device, on the host and, where it is built, in the unmodified program (two cutbacks)."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("t341_bilinear", d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    old = "!STEP, SUBSTEPS=3, CONVERG=1.0e-3\n BOUNDARY, 1\n"
    assert old in s
    with open(p, "w") as fh:
        fh.write(s.replace(old, AUTOINC))
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    dev = runs["device"]
    assert _line(341) in dev["stdout"] and dev["stdout"].count("State has been restored") >= 1
    seq = [(x[0], x[1], x[2], x[3]) for x in dev["sta"]]
    assert seq == [(x[0], x[1], x[2], x[3]) for x in runs["host"]["sta"]], (dev["sta"], runs["host"]["sta"])
    assert dev["stdout"].count("State has been restored") == runs["host"]["stdout"].count("State has been restored")
    for x, y in zip(dev["log"], runs["host"]["log"]):
        assert f1.compare_step(x, y) == []
    if f1.have("fistr1_ref"):
        r = f1.run("fistr1_ref", d, threads=2)
        assert seq == [(x[0], x[1], x[2], x[3]) for x in r["sta"]]


def test_drucker_prager_can_keeps_the_host_loops():
    """tutorial/06_plastic_can (Drucker-Prager, TYPE=342): the material is outside the kernels, no device-assembly line."""
    _need()
    r = f1.run_deck("fistr1_hip", "t06", "can.msh", "can.cnt", env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]


def test_tetrahedra_opt_in(tmp_path):
    """Without HECMW_GPU_NL_TET=1 a nonlinear tet deck keeps the host loops (the solve still runs on the device)."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("t342_elastic_tl", d)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the host" in r["stdout"]
