"""fistr1 itself (oracle/_ref/fistr1_hip) with nonlinear decks of the mixed cube: `!SOLUTION, TYPE=NLSTATIC` meshes of several of
the six solid types (361 + 351 + 341, or 362 + 352 + 342) run fstr_StiffMatrix and fstr_UpdateNewton of every Newton iteration
on the device (fx_nl_init_groups, one group per elem_type_item entry) when HECMW_GPU_NL_MIXED=1 asks for it.  The recorded decks
(tests/golden/nl_mixed_decks.npz, the unmodified program's runs; make_nl_mixed_golden.py writes the decks with
scripts/fistr1_cube_deck.py --mixed) print the report line, match the host loops (HECMW_GPU_ASSEMBLY=0) at 1e-7 and the recording
at the harness' 1e-4, with equal FSTR.sta rows; one of them runs with an `!AUTOINC_PARAM` card, device against host.  Without
the switch, with a TYPE=301 truss in the mesh, and for a single-type deck that sets only this switch, the host loops run."""
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


def _line(types):
    return ("### libfistr_hip: stiffness assembly and stress update on the device (TYPE=%s); HECMW_GPU_ASSEMBLY=0 keeps them on the host"
            % types)


def _need():
    if not f1.have("fistr1_hip"):
        pytest.skip("oracle/_ref/fistr1_hip not built (needs the reference tree at build time)")


def _golden():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_nl_mixed_golden as G
    return G


def _both(run):
    out = {}
    for mode, env in (("device", {"HECMW_GPU_NL_MIXED": "1"}), ("host", {"HECMW_GPU_ASSEMBLY": "0"})):
        r = run(dict(env, HECMW_GPU_REPORT="1"))
        assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
        assert "reference CPU solver used" not in r["stdout"]
        out[mode] = r
    return out


def _on_the_host(r):
    assert r["returncode"] == 0 and "FrontISTR Completed !!" in r["stdout"], r["stdout"][-2000:]
    assert "stiffness assembly and stress update on the device" not in r["stdout"] and "fstr_StiffMatrix on the device" not in r["stdout"]
    assert "fstr_StiffMatrix on the host" in r["stdout"]


@pytest.mark.parametrize("name", ["m%d_%s" % (order, k) for order in (1, 2)
                                  for k in ("elastic_tl", "elastic_ul", "bilinear", "multilinear_two")])
def test_recorded_mixed_decks(name, tmp_path):
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck(name, d)
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    dev, host = runs["device"]["stdout"], runs["host"]["stdout"]
    assert _line(G.TYPES[G.DECKS[name][0]]) in dev
    assert "fstr_StiffMatrix on the device" in dev and "fstr_UpdateNewton on the device" in dev
    assert "on the device (TYPE=" not in host and "fstr_StiffMatrix on the device" not in host and "fstr_UpdateNewton on the device" not in host
    a, b = runs["device"]["log"], runs["host"]["log"]
    g = np.load(os.path.join(HERE, "golden", "nl_mixed_decks.npz"))
    want = json.loads(str(g[name + "/log"]))
    assert len(a) == len(b) == len(want) >= 3
    for k, (x, y, z) in enumerate(zip(a, b, want)):
        bad = f1.compare_step(x, y, threshold=1e-7)
        print(name, "step", k, "device against host at 1e-7:", bad)
        assert bad == [], k
        assert f1.compare_step(x, z) == [], k
    assert runs["device"]["sta"] == runs["host"]["sta"]
    assert [row[3] for row in runs["device"]["sta"]] == [int(v) for v in g[name + "/newton"]]


AUTOINC = ("!AUTOINC_PARAM, NAME=AP1\n 0.25, 10, 50, 10, 1\n 1.25, 10, 1, 2, 2\n 0.5, 8\n"
           "!STEP, SUBSTEPS=40, CONVERG=1.0e-3, MAXITER=10, INC_TYPE=AUTO, AUTOINCPARAM=AP1\n 0.34, 1.0, 1.0e-6, 0.34\n BOUNDARY, 1\n")


def test_automatic_incrementation(tmp_path):
    """The Mises BILINEAR order-1 deck with the `!AUTOINC_PARAM` card of test_gpu_fistr1_tet_nonlinear.py and MAXITER=10: the
    sub-step sequence of FSTR.sta (status, Newton iterations) and the number of restored states are the same on the device and
    on the host; the cutback path rolls every group's history back (fx_nl_snapshot)."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("m1_bilinear", d)
    p = os.path.join(d, "cube.cnt")
    with open(p) as fh:
        s = fh.read()
    old = "!STEP, SUBSTEPS=3, CONVERG=1.0e-3\n BOUNDARY, 1\n"
    assert old in s
    with open(p, "w") as fh:
        fh.write(s.replace(old, AUTOINC))
    runs = _both(lambda env: f1.run("fistr1_hip", d, env=env))
    dev = runs["device"]
    assert _line(G.TYPES[1]) in dev["stdout"]
    seq = [(x[0], x[1], x[2], x[3]) for x in dev["sta"]]
    print("sub-steps", seq, "restored", dev["stdout"].count("State has been restored"))
    assert seq == [(x[0], x[1], x[2], x[3]) for x in runs["host"]["sta"]], (dev["sta"], runs["host"]["sta"])
    assert dev["stdout"].count("State has been restored") == runs["host"]["stdout"].count("State has been restored")
    for x, y in zip(dev["log"], runs["host"]["log"]):
        assert f1.compare_step(x, y) == []


def test_opt_in(tmp_path):
    """Without HECMW_GPU_NL_MIXED=1 a nonlinear mixed deck keeps the host loops, whatever the single-type switches say."""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("m2_elastic_tl", d)
    for env in ({}, {"HECMW_GPU_NL_C3": "1", "HECMW_GPU_NL_TET": "1"}):
        _on_the_host(f1.run("fistr1_hip", d, env=dict(env, HECMW_GPU_REPORT="1")))


def test_a_type_outside_the_six_keeps_the_host_loops(tmp_path):
    """The order-1 deck with one TYPE=301 truss added along an edge of the first hexahedron, as in test_gpu_fistr1_mixed.py"""
    _need()
    G = _golden()
    d = str(tmp_path / "deck")
    G.write_deck("m1_elastic_tl", d)
    msh = os.path.join(d, "cube.msh")
    s = open(msh).read()
    assert "!MATERIAL,NAME=MAT1" in s
    open(msh, "w").write(s.replace("!MATERIAL,NAME=MAT1", "!ELEMENT,TYPE=301,EGRP=E1\n23,1,2\n!MATERIAL,NAME=MAT1", 1))
    r = f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1", "HECMW_GPU_NL_MIXED": "1"})
    _on_the_host(r)
    assert len(r["sta"]) == 3


def test_single_types_keep_their_own_switches(tmp_path):
    """A 362 deck with only HECMW_GPU_NL_MIXED=1 set keeps the host loops: single types still need HECMW_GPU_NL_C3"""
    _need()
    d = str(tmp_path / "deck")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fistr1_cube_deck.py"), d, "1", "3", "--etype", "362", "--nl-material", "elastic_tl"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    _on_the_host(f1.run("fistr1_hip", d, env={"HECMW_GPU_REPORT": "1", "HECMW_GPU_NL_MIXED": "1"}))
