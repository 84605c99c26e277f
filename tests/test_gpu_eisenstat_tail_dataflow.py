"""The latency-bound tail of the Eisenstat CG + SSOR sweeps as one dataflow launch per half sweep (k_eis_backward_df /
k_eis_forward_df, FX_DATAFLOW >= 1) against the launch per colour (FX_DATAFLOW=0): the same operands in the same order per row, so
iteration count, residual history and solution are bit-identical.  Every test checks through fx_eis_tail_stats that the tail path
ran, and which colours it covered."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mesh(kind, n):
    from frontistr_amd.mesh import CubeMesh, RenumberedMesh
    if kind == "renumbered":
        return RenumberedMesh(CubeMesh(n, skew=0.1), seed=7)
    return CubeMesh(n, skew=0.2 if kind == "skewed" else 0.0)


def _solve(hip, mesh, env, monkeypatch, sigma=1.0):
    from oracle.refrun import default_params
    for k in ("FX_DATAFLOW", "FX_DF_GRID", "FX_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
    hm.elem_node_item = mesh.conn.ravel()
    m = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(m, what=hip.FX_UP_PROFILE)
    ctx.assemble_c3d8(mesh.coord, mesh.conn, 210000.0, 0.3, elemopt=1, load=mesh.load(), bc=mesh.dirichlet())
    I, R = default_params(method=1, precond=1, sigma_diag=sigma)
    m.Iarray[:] = I
    m.Rarray[:] = R
    code = ctx.solve_resident(m)
    ctx.download_x(m)
    st = ctx.stats()
    out = dict(code=code, it=ctx.info.iterations, hist=ctx.history.copy(), X=m.X.copy(), eis=st["eisenstat"],
               fallbacks=st["df_fallbacks"], tail=ctx.eis_tail_stats())
    ctx.close()
    return out


def _same(a, b):
    assert a["code"] == b["code"] == 0
    assert a["eis"] == b["eis"] == 1
    assert a["it"] == b["it"]
    assert np.array_equal(a["hist"], b["hist"])
    assert np.array_equal(a["X"], b["X"])


# (mesh, elements per edge, FX_DF_GRID, SIGMA_DIAG, tail): "part" = the tail is a strict subset of the colours (a small grid makes
# the big colours bandwidth-bound by the rule), "all" = every colour is tail
CASES = [("cube", 40, "8", 1.0, "part"), ("cube", 12, None, 1.0, "all"), ("skewed", 30, "4", 1.0, "part"),
         ("renumbered", 14, None, 1.0, "all"), ("cube", 24, "4", 1.3, "part"), ("skewed", 10, None, 1.3, "all")]


@pytest.mark.parametrize("kind,n,grid,sigma,tail", CASES)
def test_tail_dataflow_is_bit_identical(hip, monkeypatch, kind, n, grid, sigma, tail):
    mesh = _mesh(kind, n)
    env = {} if grid is None else {"FX_DF_GRID": grid}
    ref = _solve(hip, mesh, dict(env, FX_DATAFLOW="0"), monkeypatch, sigma)
    got = _solve(hip, mesh, dict(env, FX_DATAFLOW="1"), monkeypatch, sigma)
    _same(ref, got)
    assert ref["tail"]["launches"] == 0 and ref["tail"]["color0"] == ref["tail"]["ncolor"]
    t = got["tail"]
    assert t["launches"] >= 2 and got["fallbacks"] == 0           # counted when enqueued or captured into a graph
    if grid is not None:
        assert t["grid"] <= int(grid)
    if tail == "all":
        assert t["color0"] == 0
    else:
        assert 0 < t["color0"] < t["ncolor"]


@pytest.mark.parametrize("kind,n,grid", [("cube", 40, "8"), ("cube", 12, None)])
def test_tail_dataflow_graph_replay(hip, monkeypatch, kind, n, grid):
    """FX_GRAPH=2 (the iteration captured once and replayed) against FX_GRAPH=0, both with the dataflow tail, and against
    FX_DATAFLOW=0: the tags are refilled inside every replayed iteration."""
    mesh = _mesh(kind, n)
    env = {} if grid is None else {"FX_DF_GRID": grid}
    plain = _solve(hip, mesh, dict(env, FX_GRAPH="0"), monkeypatch)
    graph = _solve(hip, mesh, dict(env, FX_GRAPH="2"), monkeypatch)
    ref = _solve(hip, mesh, dict(env, FX_GRAPH="2", FX_DATAFLOW="0"), monkeypatch)
    _same(plain, graph)
    _same(ref, graph)
    assert plain["tail"]["launches"] > 0 and graph["tail"]["launches"] > 0 and ref["tail"]["launches"] == 0
    assert graph["fallbacks"] == 0


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import numpy as np
import pytest
from frontistr_amd import hecmw as hip
from test_gpu_eisenstat_tail_dataflow import _mesh, _solve
mp = pytest.MonkeyPatch()
r = _solve(hip, _mesh('cube', 12), {}, mp)
np.save(sys.argv[2], np.concatenate([np.array([r['code'], r['it'], r['fallbacks'], r['tail']['launches'], r['eis']], dtype=np.float64),
                                     r['hist'], r['X']]))
"""


def test_tail_dataflow_timeout_falls_back(hip, monkeypatch, tmp_path):
    """FX_DEBUG_DF_FAIL=1 (a fresh child process): the tail launches report a timed-out wait at once and write nothing; the solve
    is redone with a launch per colour, gives FX_DATAFLOW=0's bits, and the fallback is counted once."""
    out = str(tmp_path / "child.npy")
    env = dict(os.environ, FX_DEBUG_DF_FAIL="1")
    for k in ("FX_DATAFLOW", "FX_DF_GRID", "FX_GRAPH"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, cwd=ROOT, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    r = np.load(out)
    ref = _solve(hip, _mesh("cube", 12), {"FX_DATAFLOW": "0"}, monkeypatch)
    code, it, fallbacks, launches, eis = r[:5]
    assert code == 0 and eis == 1
    assert fallbacks == 1 and launches >= 1           # the tail ran, timed out, and the context fell back once
    nh = len(ref["hist"])
    assert it == ref["it"] and np.array_equal(r[5:5 + nh], ref["hist"]) and np.array_equal(r[5 + nh:], ref["X"])
