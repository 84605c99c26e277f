"""fistr1 itself with wedge and 20-node hexahedron decks on the device (oracle/_ref/fistr1_hip, the reference's main program
with the binding of frontistr_amd/shim/): linear static meshes of TYPE=351, 352 or 362 only run fstr_StiffMatrix through
fx_assemble_c3; fstr_UpdateNewton runs through fx_update_c3_linear with HECMW_GPU_UPDATE=1 (for these three types the device
stress update is opt-in: DESIGN.md section 4 has the timings that decided it).

Must fail without the feature: before the binding admitted these types no run printed the report line
`### libfistr_hip: stiffness assembly on the device (linear static, TYPE=351|352|362)`; the element loops stayed on the host.

The reference's own static regression decks of these types (exA/B/C/D/E and exG) print the device line and match their
*_correct.log (examples/test_FrontISTR.rb's 1e-4) and the same program with HECMW_GPU_ASSEMBLY=0 (1e-7, the bound of
test_gpu_fistr1_tet.py); the thermal exF decks keep the host loops; the synthetic cube decks of scripts/fistr1_cube_deck.py
--etype match the host loops and the unmodified program's extrema recorded in tests/golden/c3_decks.npz
(make_c3_golden.py)."""
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


def _c3_models():
    with open(os.path.join(f1.DECKS, "static", "manifest.json")) as fh:
        return [tuple(x) for x in json.load(fh) if x[1][1:] in ("351", "352", "362")]


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (build() makes it where the reference sources are present)")


def _both(run):
    """run(env) on the device (default: assembly there, stress update on the host), with HECMW_GPU_UPDATE=1 (both there) and with
    HECMW_GPU_ASSEMBLY=0; all must complete."""
    out = {}
    for mode, env in (("device", {}), ("update", {"HECMW_GPU_UPDATE": "1"}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


@pytest.mark.parametrize("sub,model,mesh,cnt,ndof", [m for m in _c3_models() if m[0] != "exF"], ids=lambda v: str(v))
def test_static_c3_decks_assemble_on_the_device(sub, model, mesh, cnt, ndof):
    _need()
    etype = int(model[1:])
    runs = _both(lambda env: f1.run_deck("fistr1_hip", os.path.join("static", sub), mesh, cnt, env=env))
    dev, upd, host = runs["device"]["stdout"], runs["update"]["stdout"], runs["host"]["stdout"]
    assert _line(etype) in dev and "fstr_StiffMatrix on the device" in dev and "fstr_UpdateNewton on the host" in dev
    assert _line(etype) in upd and "fstr_StiffMatrix on the device" in upd and "fstr_UpdateNewton on the device" in upd
    assert "stiffness assembly on the device" not in host and "fstr_StiffMatrix on the host" in host
    correct = f1.read_log(os.path.join(f1.DECKS, "static", sub, model + "_correct.log"))
    b = runs["host"]["log"][-1]
    for mode in ("device", "update"):
        a = runs[mode]["log"][-1]
        assert correct and f1.compare_step(a, correct[-1]) == [], mode
        assert f1.compare_step(a, b, threshold=1e-7) == [], mode


@pytest.mark.parametrize("model,mesh,cnt", [(m[1], m[2], m[3]) for m in _c3_models() if m[0] == "exF"])
def test_thermal_c3_decks_stay_on_the_host(model, mesh, cnt):
    _need()
    r = f1.run_deck("fistr1_hip", os.path.join("static", "exF"), mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    correct = f1.read_log(os.path.join(f1.DECKS, "static", "exF", model + "_correct.log"))
    assert f1.compare_step(r["log"][-1], correct[-1]) == []


CUBES = [("c351_n2", 351, 2, False), ("c351_n2_two", 351, 2, True), ("c352_n2", 352, 2, False), ("c352_n2_two", 352, 2, True),
         ("c362_n2", 362, 2, False), ("c362_n2_two", 362, 2, True), ("c351_n5", 351, 5, False), ("c352_n4", 352, 4, False),
         ("c362_n4", 362, 4, False)]


@pytest.mark.parametrize("name,etype,n,two", CUBES, ids=[c[0] for c in CUBES])
def test_c3_cube_decks(name, etype, n, two, tmp_path):
    """The cube decks of fistr1_cube_deck.py --linear --etype: device against HECMW_GPU_ASSEMBLY=0 at 1e-7, and against the unmodified
    program's 0.log where make_c3_golden.py recorded it."""
    _need()
    d = str(tmp_path / "deck")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, str(n), "--linear", "--etype", str(etype)]
    subprocess.run(cmd + (["--two-sections"] if two else []), check=True, stdout=subprocess.DEVNULL)
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    assert _line(etype) in runs["device"]["stdout"] and "fstr_UpdateNewton on the host" in runs["device"]["stdout"]
    assert _line(etype) in runs["update"]["stdout"] and "fstr_UpdateNewton on the device" in runs["update"]["stdout"]
    b = runs["host"]["log"][-1]
    g = np.load(os.path.join(HERE, "golden", "c3_decks.npz"))
    ref = None
    if name + "/log" in g:
        ref = json.loads(str(g[name + "/log"]))
    elif f1.have("fistr1_ref"):
        ref = f1.run("fistr1_ref", d, threads=2)["log"][-1]
    for mode in ("device", "update"):
        a = runs[mode]["log"][-1]
        assert len(a["Node"]) >= 10 and f1.compare_step(a, b, threshold=1e-7) == [], mode
        if ref is not None:
            assert f1.compare_step(a, ref) == [], mode
