"""fistr1 itself (oracle/_ref/fistr1_hip) with `!VISCOELASTIC` and `!CREEP` decks: with HECMW_GPU_NL_VISCO=1 fstr_StiffMatrix and
fstr_UpdateNewton of every Newton iteration and fstr_UpdateState of every sub-step run on the device (material kinds 7 / 8 of
fx_material_view; ctime and tincr of every call through fx_nl_set_time; the whole fstatus(:) of such points both ways); without the
switch the host loops run.  Decks: tutorial/07_viscoelastic_cylinder and 08_creep_cylinder (tests/golden/decks/t07, t08; 08 has no
`TYPE=VISCO` step, so its creep never acts and what runs is the ELASTIC arithmetic plus the latch), the reference's
examples/static/1elem/{relax,viscoe,viscof,creep} (tests/golden/decks/visco1) and two recorded cube decks with their type gates.
They report the element loops on the device with `, viscoelastic` / `, creep` and reproduce the Newton counts of FSTR.sta and the
Global summaries of 0.log that the unmodified program recorded, at the reference harness's 1e-4.

1elem/creep: the unmodified program stops in the first VISCO increment at ITMAX = 20 (tests/golden/make_visco_golden.py says why);
with the device loops the program stops the same way after the same counts.

No recorded deck of these materials has a cutback or a restart; none is run here."""
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
SWITCH = {"HECMW_GPU_NL_VISCO": "1", "HECMW_GPU_REPORT": "1"}


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_visco_golden as G
    return G


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _report(out, on_device, word):
    lines = [l for l in out.split("\n") if DEVICE in l]
    assert (len(lines) == 1) == on_device, lines
    if on_device:
        assert lines[0].rstrip().endswith(word), lines[0]
    assert ("fstr_StiffMatrix on the device" in out) == on_device and ("fstr_UpdateNewton on the device" in out) == on_device


def _check(r, want, newton, on_device, word, completes=True):
    assert ("FrontISTR Completed !!" in r["stdout"]) == completes, r["stdout"][-2000:]
    if completes:
        assert r["returncode"] == 0
    else:
        assert "Fail to Converge" in r["stdout"]
    assert "reference CPU solver used" not in r["stdout"]
    _report(r["stdout"], on_device, word)
    assert [row[3] for row in r["sta"]] == newton, (r["sta"], newton)
    assert len(r["log"]) == len(want)
    for k, (a, c) in enumerate(zip(r["log"], want)):
        assert H.within_1e4(a, c) == [], k


def _recorded(name):
    g = np.load(os.path.join(HERE, "golden", "visco_decks.npz"))
    return json.loads(str(g[name + "/log"])), [int(v) for v in g[name + "/newton"]]


@pytest.mark.parametrize("deck,word", [("t07", ", viscoelastic"), ("t08", ", creep")])
def test_tutorials_on_the_device(deck, word):
    _need()
    want = f1.read_log(os.path.join(f1.DECKS, deck, "cylinder_fistr1_ref_0.log"))
    newton = [row[3] for row in f1.read_sta(os.path.join(f1.DECKS, deck, "cylinder_fistr1_ref_FSTR.sta"))]
    r = f1.run_deck("fistr1_hip", deck, "cylinder.msh", "cylinder.cnt", env=SWITCH)
    _check(r, want, newton, True, word)
    if deck == "t07":       # without the switch: the host loops
        r = f1.run_deck("fistr1_hip", deck, "cylinder.msh", "cylinder.cnt", env={"HECMW_GPU_REPORT": "1"})
        _check(r, want, newton, False, word)


@pytest.mark.parametrize("name,word", [("1elem_relax", ", creep"), ("1elem_viscoe", ", viscoelastic"), ("1elem_viscof", ", viscoelastic"),
                                       ("1elem_creep", ", creep")])
def test_reference_one_element_decks_on_the_device(name, word):
    _need()
    deck, mesh, cnt = _golden().REFERENCE_DECKS[name]
    want, newton = _recorded(name)
    r = f1.run_deck("fistr1_hip", deck, mesh, cnt, env=SWITCH)
    _check(r, want, newton, True, word, completes=name != "1elem_creep")
    if name == "1elem_relax":
        r = f1.run_deck("fistr1_hip", deck, mesh, cnt, env={"HECMW_GPU_REPORT": "1"})
        _check(r, want, newton, False, word)


@pytest.mark.parametrize("name,gate,word", [("v342_norton_two", "HECMW_GPU_NL_TET", ", creep"), ("v362_visco", "HECMW_GPU_NL_C3", ", viscoelastic"),
                                            ("v361_visco_fbar", "HECMW_GPU_NL_FBAR", ", viscoelastic")])
def test_recorded_cube_decks(name, gate, word, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    want, newton = _recorded(name)
    r = f1.run("fistr1_hip", d, env=dict(SWITCH, **{gate: "1"}))
    _check(r, want, newton, True, word)
    # the type's own gate still applies, and so does this one
    r = f1.run("fistr1_hip", d, env=SWITCH)
    _check(r, want, newton, False, word)
    r = f1.run("fistr1_hip", d, env={gate: "1", "HECMW_GPU_REPORT": "1"})
    _check(r, want, newton, False, word)
