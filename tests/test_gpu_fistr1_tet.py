"""fistr1 itself with tetrahedral decks on the device (oracle/_ref/fistr1_hip, the reference's main program with the binding of
frontistr_amd/shim/): linear static meshes of TYPE=341 or 342 only run fstr_StiffMatrix through fx_assemble_c3 and
fstr_UpdateNewton through fx_update_c3_linear.  The reference's own static regression decks of these types (exA/B/C/D/E and
exG) print the device line and match their *_correct.log (examples/test_FrontISTR.rb's 1e-4) and the same program with
HECMW_GPU_ASSEMBLY=0 (1e-7); the thermal exF decks keep the host loops; the synthetic tet cube decks of
scripts/fistr1_cube_deck.py --etype match the host loops and the unmodified program's extrema recorded in
tests/golden/tet_decks.npz (make_tet_golden.py)."""
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


def _line(etype):
    return "### libfistr_hip: stiffness assembly on the device (linear static, TYPE=%d); HECMW_GPU_ASSEMBLY=0 keeps it on the host" % etype


def _tet_models():
    with open(os.path.join(f1.DECKS, "static", "manifest.json")) as fh:
        return [tuple(x) for x in json.load(fh) if x[1][1:] in ("341", "342")]


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs /root/reference at build time)")


def _both(run):
    """run(env) on the device and with HECMW_GPU_ASSEMBLY=0; both must complete."""
    out = {}
    for mode, env in (("device", {}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


@pytest.mark.parametrize("sub,model,mesh,cnt,ndof", [m for m in _tet_models() if m[0] != "exF"], ids=lambda v: str(v))
def test_static_tet_decks_assemble_on_the_device(sub, model, mesh, cnt, ndof):
    _need()
    etype = int(model[1:])
    runs = _both(lambda env: f1.run_deck("fistr1_hip", os.path.join("static", sub), mesh, cnt, env=env))
    dev, host = runs["device"]["stdout"], runs["host"]["stdout"]
    assert _line(etype) in dev and "fstr_StiffMatrix on the device" in dev and "fstr_UpdateNewton on the device" in dev
    assert "stiffness assembly on the device" not in host and "fstr_StiffMatrix on the host" in host
    correct = f1.read_log(os.path.join(f1.DECKS, "static", sub, model + "_correct.log"))
    a, b = runs["device"]["log"][-1], runs["host"]["log"][-1]
    assert correct and f1.compare_step(a, correct[-1]) == []
    assert f1.compare_step(a, b, threshold=1e-7) == []


@pytest.mark.parametrize("model,mesh,cnt", [(m[1], m[2], m[3]) for m in _tet_models() if m[0] == "exF"])
def test_thermal_tet_decks_stay_on_the_host(model, mesh, cnt):
    _need()
    r = f1.run_deck("fistr1_hip", os.path.join("static", "exF"), mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    correct = f1.read_log(os.path.join(f1.DECKS, "static", "exF", model + "_correct.log"))
    assert f1.compare_step(r["log"][-1], correct[-1]) == []


CUBES = [("t341_n2", 341, 2, False), ("t341_n2_two", 341, 2, True), ("t342_n1", 342, 1, False), ("t342_n1_two", 342, 1, True),
         ("t342_n4", 342, 4, False)]


@pytest.mark.parametrize("name,etype,n,two", CUBES, ids=[c[0] for c in CUBES])
def test_tet_cube_decks(name, etype, n, two, tmp_path):
    """The cube decks of fistr1_cube_deck.py --linear --etype: device against HECMW_GPU_ASSEMBLY=0 at 1e-7, and against the unmodified
    program's 0.log where make_tet_golden.py recorded it."""
    _need()
    d = str(tmp_path / "deck")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, str(n), "--linear", "--etype", str(etype)]
    subprocess.run(cmd + (["--two-sections"] if two else []), check=True, stdout=subprocess.DEVNULL)
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    assert _line(etype) in runs["device"]["stdout"] and "fstr_UpdateNewton on the device" in runs["device"]["stdout"]
    a, b = runs["device"]["log"][-1], runs["host"]["log"][-1]
    assert len(a["Node"]) >= 10 and f1.compare_step(a, b, threshold=1e-7) == []
    g = np.load(os.path.join(HERE, "golden", "tet_decks.npz"))
    if name + "/log" in g:
        assert f1.compare_step(a, json.loads(str(g[name + "/log"]))) == []
    elif f1.have("fistr1_ref"):
        assert f1.compare_step(a, f1.run("fistr1_ref", d, threads=2)["log"][-1]) == []
