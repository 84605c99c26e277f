"""Block ILU(0) (PRECOND = 10) on the generic-block path, NDOF = 4, 5, 6, against the reference's own vectors
(tests/golden/nn_ilu.npz, NDOF 5 and 6) and the numpy restatement tests/nn_ilu_ref.py (NDOF 4, and wide rows).
Before this preconditioner existed, every solve and apply here failed with E-1001."""
import numpy as np
import pytest

import nn_ilu_ref
from conftest import load_golden
from nn_cases import dense, nn_system, wide_system

pytestmark = pytest.mark.gpu


def to_hip(hip, A, meth=1, pc=10):
    m = hip.hecmwST_matrix.from_arrays(A.N, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, A.B.copy(),
                                       NDOF=A.NDOF)
    m.Iarray[0], m.Iarray[1], m.Iarray[2] = 10000, meth, pc
    return m


def expected_z(A, k=0):
    if A.NDOF in (5, 6) and A.N == nn_system(A.NDOF).N:
        return load_golden("nn_ilu")["z_n%d_s%d" % (A.NDOF, k)]
    sig = float(load_golden("nn_ilu")["sigmas"][k])
    return nn_ilu_ref.apply(A, nn_ilu_ref.factor(A, sig), A.B)


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("nd", [4, 5, 6])
@pytest.mark.parametrize("k", [0, 1])
def test_apply_matches_reference(hip, nd, k):
    A = nn_system(nd)
    m = to_hip(hip, A)
    m.Rarray[1] = float(load_golden("nn_ilu")["sigmas"][k])
    ctx = hip.SolverContext()
    z = ctx.nn_precond_apply(m, A.B)
    st = ctx.nn_precond_stats()
    assert st["kind"] == 10 and st["factor_lanes"] == 32 and st["levels"] > 1 and st["max_row_blocks"] == 26
    assert rel(z, expected_z(A, k)) <= 1e-12
    z2 = hip.SolverContext().nn_precond_apply(to_hip(hip, A), A.B) if k == 0 else None
    if z2 is not None:
        assert np.array_equal(z, z2)            # two fresh contexts: the same bits
    ctx.close()


@pytest.mark.parametrize("nd", [4, 5, 6])
def test_apply_wide_rows_one_thread_factor(hip, nd):
    A = wide_system(nd)
    ctx = hip.SolverContext()
    z = ctx.nn_precond_apply(to_hip(hip, A), A.B)
    st = ctx.nn_precond_stats()
    assert st["factor_lanes"] == 1 and st["max_row_blocks"] > 32
    assert rel(z, nn_ilu_ref.apply(A, nn_ilu_ref.factor(A), A.B)) <= 1e-12
    ctx.close()


@pytest.mark.parametrize("nd", [5, 6])
@pytest.mark.parametrize("meth", [1, 2, 3, 4])
def test_solve_vs_reference(hip, nd, meth):
    g = load_golden("nn_ilu")
    tag = "n%d_m%d_" % (nd, meth)
    m = to_hip(hip, nn_system(nd), meth)
    ctx = hip.SolverContext()
    assert hip.hecmw_solve(None, m, ctx=ctx) == 0 and m.Iarray[80] == 1
    assert abs(ctx.info.iterations - int(g[tag + "iter"])) <= 1
    assert rel(m.X, g[tag + "X"]) <= 1e-8
    ctx.close()


@pytest.mark.parametrize("meth", [1, 2, 3, 4])
def test_solve_ndof4(hip, meth):
    A = nn_system(4)
    m = to_hip(hip, A, meth)
    ctx = hip.SolverContext()
    assert hip.hecmw_solve(None, m, ctx=ctx) == 0 and m.Iarray[80] == 1
    assert rel(m.X, np.linalg.solve(dense(A), A.B)) <= 1e-6
    ctx.close()


@pytest.mark.parametrize("tag,nd,meth,scaling,ipm", [("n6_scal_", 6, 1, 1, 1), ("n5_ipm2_", 5, 2, 0, 2)])
def test_scaling_and_iterpremax(hip, tag, nd, meth, scaling, ipm):
    g = load_golden("nn_ilu")
    m = to_hip(hip, nn_system(nd), meth)
    m.Iarray[6], m.Iarray[4] = scaling, ipm
    ctx = hip.SolverContext()
    assert hip.hecmw_solve(None, m, ctx=ctx) == 0
    assert abs(ctx.info.iterations - int(g[tag + "iter"])) <= 1
    assert rel(m.X, g[tag + "X"]) <= 1e-8
    ctx.close()


def test_sigma_diag_retry(hip):
    """SIGMA_DIAG = -1: the reference retries with SIGMA_DIAG + 0.1 up to 2, keeping the first attempt's factors and restarting
    from the X the failed attempt left (hecmw_solver_Iterative.f90:145-156)."""
    g = load_golden("nn_ilu")
    nd, blk, scale = g["retry_case"]
    nd, blk = int(nd), int(blk)
    A = nn_system(nd)
    A.D = A.D.copy()
    A.D[nd * nd * blk:nd * nd * (blk + 1)] *= scale
    m = to_hip(hip, A)
    m.Iarray[0], m.Rarray[1] = 500, -1.0
    ctx = hip.SolverContext()
    hip.hecmw_solve(None, m, ctx=ctx)
    att = ctx.solve_attempts()
    assert len(att) == int(g["retry_n_attempts"])
    assert att[0][2] == int(g["retry_attempts"][0])
    assert [round(a[1], 6) for a in att] == [round(1.0 + 0.1 * k, 6) for k in range(len(att))]
    assert ctx.info.iterations == int(g["retry_iter"]) and m.Iarray[81] == 1 and m.Iarray[80] == g["retry_Iarray"][80]
    assert rel(m.X, g["retry_X"]) <= 1e-8
    ctx.close()


def test_kind_switch_rebuilds(hip):
    """SSOR -> ILU(0) -> SSOR -> DIAG on one context: each solve gives what a fresh context gives."""
    A = nn_system(6)
    ctx = hip.SolverContext()
    for pc in (1, 10, 1, 3, 10):
        m = to_hip(hip, A, 1, pc)
        assert hip.hecmw_solve(None, m, ctx=ctx) == 0
        f = to_hip(hip, A, 1, pc)
        fresh = hip.SolverContext()
        assert hip.hecmw_solve(None, f, ctx=fresh) == 0
        assert np.array_equal(m.X, f.X), pc
        fresh.close()
    ctx.close()


def test_still_refused(hip):
    """PRECOND 10 with NDOF 1 / 2 and PRECOND 11 / 12 at every generic size stay E-1001."""
    for nd, pc in [(1, 10), (2, 10)] + [(nd, pc) for nd in (1, 2, 4, 5, 6) for pc in (11, 12)]:
        m = to_hip(hip, nn_system(nd), 1, pc)
        ctx = hip.SolverContext()
        with pytest.raises(hip.HecmwSolverError) as e:
            hip.hecmw_solve(None, m, ctx=ctx)
        assert e.value.code == hip.HECMW_SOLVER_ERROR_INCONS_PC, (nd, pc)
        ctx.close()


def test_recycle_sequence(hip):
    """ref_solve mode 4 at NDOF 6: six solves, D grows by 10 % and Iarray(97) = 1 before solves 2-6, X reset each time."""
    g = load_golden("nn_ilu")
    A = nn_system(6)
    m = to_hip(hip, A)
    x0 = m.X.copy()
    ctx = hip.SolverContext()
    iters = []
    for k in range(6):
        if k > 0:
            m.D = m.D * 1.1
            m.X = x0.copy()
            m.Iarray[96], m.Iarray[97] = 1, 0
        assert hip.hecmw_solve(None, m, ctx=ctx) == 0
        iters.append(ctx.info.iterations)
    assert all(abs(a - b) <= 1 for a, b in zip(iters, g["recycle_iters"])), (iters, g["recycle_iters"])
    assert rel(m.X, g["recycle_X"]) <= 1e-8
    ctx.close()


@pytest.mark.parametrize("nd", [4, 5, 6])
def test_dataflow_and_per_level_sweeps_bitwise(hip, nd):
    """One persistent dataflow launch (the default) and one launch per level give the same bits, also on wide rows."""
    for A in (nn_system(nd), wide_system(nd)):
        a = hip.SolverContext()
        za = a.nn_precond_apply(to_hip(hip, A), A.B)
        st = a.nn_precond_stats()
        assert st["dataflow"] == 1 and 1 <= st["df_grid"] <= st["slices"] and st["df_fallbacks"] == 0
        b = hip.SolverContext()
        b.set_option("FX_DATAFLOW", 0)
        zb = b.nn_precond_apply(to_hip(hip, A), A.B)
        assert b.nn_precond_stats()["dataflow"] == 0
        assert np.array_equal(za, zb)
        assert rel(za, nn_ilu_ref.apply(A, nn_ilu_ref.factor(A), A.B)) <= 1e-12
        a.close()
        b.close()


def test_live_dataflow_switch(hip):
    """FX_DATAFLOW flipped on a live context (both ways) gives a fresh context's bits, for applies and solves."""
    A = nn_system(5)
    fresh = hip.SolverContext()
    z0 = fresh.nn_precond_apply(to_hip(hip, A), A.B)
    m0 = to_hip(hip, A, 2)
    assert hip.hecmw_solve(None, m0, ctx=fresh) == 0
    ctx = hip.SolverContext()
    for v in (0, 1, 0):
        ctx.set_option("FX_DATAFLOW", v)
        assert np.array_equal(ctx.nn_precond_apply(to_hip(hip, A), A.B), z0)
        m = to_hip(hip, A, 2)
        assert hip.hecmw_solve(None, m, ctx=ctx) == 0
        assert np.array_equal(m.X, m0.X) and ctx.info.iterations == fresh.info.iterations
    ctx.close()
    fresh.close()


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']
from frontistr_amd import hecmw as hip
from nn_cases import nn_system
from test_gpu_nn_ilu import to_hip
A = nn_system(6)
ctx = hip.SolverContext()
z = ctx.nn_precond_apply(to_hip(hip, A), A.B)
st = ctx.nn_precond_stats()
ctx.close()
out = [z]
for meth in (1, 3):
    ctx = hip.SolverContext()
    m = to_hip(hip, A, meth)
    assert hip.hecmw_solve(None, m, ctx=ctx) == 0
    out.append(m.X)
    out.append(np.array([ctx.info.iterations, ctx.nn_precond_stats()["df_fallbacks"]], dtype=np.float64))
    ctx.close()
np.save(sys.argv[2], np.concatenate([np.array([st["df_fallbacks"], st["dataflow"]], dtype=np.float64)] + out))
"""


def test_dataflow_timeout_falls_back(hip, tmp_path):
    """FX_DEBUG_DF_FAIL=1 (a fresh child process): every dataflow sweep reports a timed-out wait at once; the apply and the
    CG / GMRES attempts are redone with per-level launches and give the default path's bits, and the fallback is counted."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "child.npy")
    env = dict(os.environ, FX_DEBUG_DF_FAIL="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, root, out], env=env, cwd=root, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    r = np.load(out)
    A = nn_system(6)
    n = 6 * A.NP
    assert r[0] == 1 and r[1] == 0                    # one fallback, the context then sweeps per level
    ctx = hip.SolverContext()
    assert np.array_equal(r[2:2 + n], ctx.nn_precond_apply(to_hip(hip, A), A.B))
    ctx.close()
    off = 2 + n
    for meth in (1, 3):
        ctx = hip.SolverContext()
        m = to_hip(hip, A, meth)
        assert hip.hecmw_solve(None, m, ctx=ctx) == 0
        assert np.array_equal(r[off:off + n], m.X) and r[off + n] == ctx.info.iterations
        assert r[off + n + 1] == 1                    # the child's attempt was redone once, from the X it started with
        ctx.close()
        off += n + 2
