"""fistr1 itself (oracle/_ref/fistr1_hip) with F-bar hexahedra (`!SECTION, FORM361=FBAR`): with HECMW_GPU_NL_FBAR=1 fstr_StiffMatrix and
fstr_UpdateNewton of every Newton iteration run on the device through fx_nl_init_groups with elemopt 4; without the switch, with an
UPDATELAG material in an F-bar section, or with B-bar and F-bar sections in one mesh the host loops run.  Decks: the reference's
examples/static/FbarElement/T01_BEAM_HYPERELASTIC and T02_BEAM_HYPOELA (committed copies under tests/golden/decks/static/FbarElement)
and the recorded cube decks of tests/golden/nl_fbar_decks.npz, rebuilt from scripts/fistr1_cube_deck.py --form361 FBAR.

Bounds: the reference harness's 1e-4 against the unmodified program's recorded summaries and the decks' own _correct.log; 1e-7 between
the device loops and the host loops of the same binary (HECMW_GPU_ASSEMBLY=0: the reference's own element code, the same device
Krylov solver), which on the five digits a log prints asks for the same digits."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DECK = "static/FbarElement"
FBAR_LINE = ("### libfistr_hip: stiffness assembly and stress update on the device (TYPE=361 F-bar); "
             "HECMW_GPU_ASSEMBLY=0 keeps them on the host")
DEVICE = "### libfistr_hip: stiffness assembly and stress update on the device"
ON = {"HECMW_GPU_NL_FBAR": "1", "HECMW_GPU_NL_HYPER": "1", "HECMW_GPU_REPORT": "1"}


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_nl_fbar_golden as G
    return G


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _ran(r):
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "reference CPU solver used" not in r["stdout"]


def _on_device(r, yes):
    out = r["stdout"]
    assert (FBAR_LINE in out) == yes and (DEVICE in out) == yes, out[-2000:]
    assert ("fstr_StiffMatrix on the device" in out) == yes and ("fstr_UpdateNewton on the device" in out) == yes


def _same(a, b, bound):
    assert len(a) == len(b) and len(a) >= 1
    for k, (x, y) in enumerate(zip(a, b)):
        assert f1.compare_step(x, y, bound) == [], k


def _recorded(name):
    g = np.load(os.path.join(HERE, "golden", "nl_fbar_decks.npz"))
    return json.loads(str(g[name + "/log"])), [int(v) for v in g[name + "/newton"]]


def test_t01_beam_hyperelastic_on_the_device():
    _need()
    name = "T01_BEAM_HYPERELASTIC"
    dev = f1.run_deck("fistr1_hip", DECK, name + ".msh", name + ".cnt", env=ON)
    _ran(dev)
    _on_device(dev, True)
    correct = f1.read_log(os.path.join(HERE, "golden", "decks", DECK, name + "_correct.log"))
    _same(dev["log"], correct, 1e-4)
    want, newton = _recorded(name)
    _same(dev["log"], want, 1e-4)
    assert [row[3] for row in dev["sta"]] == newton
    host = f1.run_deck("fistr1_hip", DECK, name + ".msh", name + ".cnt", env=dict(ON, HECMW_GPU_ASSEMBLY="0"))
    _ran(host)
    _on_device(host, False)
    _same(dev["log"], host["log"], 1e-7)
    assert dev["sta"] == host["sta"], (dev["sta"], host["sta"])


@pytest.mark.parametrize("name", ["f361_elastic_tl", "f361_neohooke", "f361_mooney", "f361_arruda", "f361_mooney_two"])
def test_recorded_cube_decks(name, tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck(name, d)
    dev = f1.run("fistr1_hip", d, env=ON)
    _ran(dev)
    _on_device(dev, True)
    host = f1.run("fistr1_hip", d, env=dict(ON, HECMW_GPU_ASSEMBLY="0"))
    _ran(host)
    _on_device(host, False)
    _same(dev["log"], host["log"], 1e-7)
    want, newton = _recorded(name)
    _same(dev["log"], want, 1e-4)
    assert [row[3] for row in dev["sta"]] == newton and [row[3] for row in host["sta"]] == newton


def test_without_the_switch_the_host_loops_run(tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck("f361_mooney", d)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_NL_HYPER": "1", "HECMW_GPU_REPORT": "1"})
    _ran(r)
    _on_device(r, False)
    assert "fstr_StiffMatrix on the host" in r["stdout"] and "fstr_UpdateNewton on the host" in r["stdout"]
    want, newton = _recorded("f361_mooney")
    _same(r["log"], want, 1e-4)


def test_updatelag_fbar_stays_on_the_host():
    """T02_BEAM_HYPOELA: `!ELASTIC, CAUCHY` on F-bar sections -- the branch of Update_C3D8Fbar that the device does not restate"""
    _need()
    name = "T02_BEAM_HYPOELA"
    r = f1.run_deck("fistr1_hip", DECK, name + ".msh", name + ".cnt", env=ON)
    _ran(r)
    _on_device(r, False)
    correct = f1.read_log(os.path.join(HERE, "golden", "decks", DECK, name + "_correct.log"))
    _same(r["log"], correct, 1e-4)


def test_bbar_and_fbar_sections_in_one_mesh_stay_on_the_host(tmp_path):
    _need()
    d = str(tmp_path / "deck")
    _golden().write_deck("f361_mooney_two", d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    assert s.count("!SECTION, SECNUM=2, FORM361=FBAR") == 1
    with open(p, "w") as fh:
        fh.write(s.replace("!SECTION, SECNUM=2, FORM361=FBAR", "!SECTION, SECNUM=2, FORM361=BBAR"))
    r = f1.run("fistr1_hip", d, env=ON)
    _ran(r)
    _on_device(r, False)
