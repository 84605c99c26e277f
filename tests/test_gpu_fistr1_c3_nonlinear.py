"""fistr1 itself (oracle/_ref/fistr1_hip) with nonlinear decks of wedges or 20-node hexahedra: `!STATIC, TYPE=NLGEOM` meshes of
TYPE=351, 352 or 362 only run fstr_StiffMatrix and fstr_UpdateNewton of every Newton iteration on the device (fx_nl_init_type)
when HECMW_GPU_NL_C3=1 asks for it (these types opt in; without the switch the host loops run).  The reference's exI decks
A351 / A352 / A362 under I300.cnt (10 sub-steps, total Lagrange) print the device line, match their *_correct.log at the
reference harness's 1e-4 in every step and the same program with HECMW_GPU_ASSEMBLY=0 at 1e-7, with equal Newton counts per
sub-step; the recorded cube decks (tests/golden/nl_c3_decks.npz) match the host loops at 1e-7, the unmodified program's run at
1e-4 and its Newton counts; a thermal deck keeps the host loops."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import fistr1_run as f1

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _line(etype):
    return ("### libfistr_hip: stiffness assembly and stress update on the device (TYPE=%d); HECMW_GPU_ASSEMBLY=0 keeps them on the host"
            % etype)


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _both(run):
    out = {}
    for mode, env in (("device", {"HECMW_GPU_NL_C3": "1"}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


@pytest.mark.parametrize("etype", [351, 352, 362])
def test_exI_on_the_device(etype):
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
    import make_nl_c3_golden as G
    return G


@pytest.mark.parametrize("name", ["c%d_%s" % (et, k) for et in (351, 352, 362)
                                  for k in ("elastic_tl", "elastic_ul", "bilinear", "multilinear_two")])
def test_recorded_cube_decks(name, tmp_path):
    """The recorded cube decks (tests/golden/make_nl_c3_golden.py writes them with scripts/fistr1_cube_deck.py): the device run
    against the host loops at 1e-7, against the unmodified program's summaries in nl_c3_decks.npz at 1e-4, and the FSTR.sta rows
    with the Newton count of every sub-step equal in all three."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck(name, d)
    etype = G.DECKS[name][0]
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    assert _line(etype) in runs["device"]["stdout"] and "fstr_UpdateNewton on the device" in runs["device"]["stdout"]
    assert "on the device (TYPE=" not in runs["host"]["stdout"]
    a, b = runs["device"]["log"], runs["host"]["log"]
    g = np.load(os.path.join(HERE, "golden", "nl_c3_decks.npz"))
    want = json.loads(str(g[name + "/log"]))
    assert len(a) == len(b) == len(want) >= 3
    for k, (x, y, z) in enumerate(zip(a, b, want)):
        bad = f1.compare_step(x, y, threshold=1e-7)
        print(name, "step", k, "device against host at 1e-7:", bad)
        assert bad == [], k
        assert f1.compare_step(x, z) == [], k
    assert runs["device"]["sta"] == runs["host"]["sta"]
    assert [row[3] for row in runs["device"]["sta"]] == [int(v) for v in g[name + "/newton"]]


def test_opt_in(tmp_path):
    """Without HECMW_GPU_NL_C3=1 a nonlinear 362 deck keeps the host loops (the solve still runs on the device); HECMW_GPU_NL_TET=1
    admits the tetrahedra only."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("c362_elastic_tl", d)
    for env in ({}, {"HECMW_GPU_NL_TET": "1"}):
        r = f1.run("fistr1_hip", d, env=dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the host" in r["stdout"]


def test_thermal_deck_keeps_the_host_loops(tmp_path):
    """An NLGEOM 352 deck with a `!TEMPERATURE` load (the elastic total-Lagrange cube with an expansion coefficient and 10 degrees
    on the top face): the nonlinear gate's thermal test keeps the host loops even with HECMW_GPU_NL_C3=1."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("c352_elastic_tl", d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    step, elastic = "!STEP, SUBSTEPS=3, CONVERG=1.0e-3\n BOUNDARY, 1\n", "!ELASTIC\n 206900.0, 0.29\n"
    assert step in s and elastic in s
    s = s.replace(step, "!TEMPERATURE\n TOP, 10.0\n!REFTEMP\n 0.0\n" + step).replace(elastic, elastic + "!EXPANSION_COEFF\n 1.0e-5\n")
    with open(p, "w") as fh:
        fh.write(s)
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1", "HECMW_GPU_NL_C3": "1"})
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    assert "fstr_StiffMatrix on the host" in r["stdout"] and len(r["sta"]) == 3
    if f1.have("fistr1_ref"):
        ref = f1.run("fistr1_ref", d, threads=2)
        assert f1.compare_step(r["log"][-1], ref["log"][-1]) == []
