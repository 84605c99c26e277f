"""The generic-block path (NDOF = 1, 2, 4, 5, 6) at sizes where its kernels leave the one-workgroup cases, against the fp64 CPU
oracle (bit-identical to the reference on the small systems: tests/test_oracle_nn.py, tests/test_oracle_nn_ilu.py):
  cube20  20^3 hex8 (9,261 nodes): SSOR colours of up to 19 slices, 1 and 63 rows mod 64, partly filled last workgroups; 141
          ILU levels in 218 slices, 77 of them over one slice
  random  3,000 rows of a random profile: halo columns, isolated rows, a hub row of 65 blocks (the one-thread factor), levels
          over 128 rows, off-diagonal blocks that are not symmetric
  big     NDOF * N > 2048 x 256: the grid-stride loops of the Krylov vector kernels, more than 256 partials in k_nn_reduce
What each shape reaches is checked from the profile alone in tests/test_nn_shapes.py.  Bounds as tests/test_gpu_nn.py and
tests/test_gpu_nn_ilu.py: SpMV 1e-13, preconditioner applies 1e-12, CG / BiCGSTAB iterations +-1 and X 1e-8, GMRES / GPBiCG
iterations +-10 % and X 1e-7 (relative to the largest entry)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from nn_cases import SHAPE_NDOF, SSOR_NCOLOR, shape_system

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL = ("cube20", "random")


@pytest.fixture(scope="module")
def systems():
    """Each shape is built once per module (the big ones only when a test asks for them)."""
    cache = {}

    def get(name, nd):
        if (name, nd) not in cache:
            if name == "big":                  # keep host memory modest: one big system at a time
                for k in [k for k in cache if k[0] == "big"]:
                    del cache[k]
            cache[(name, nd)] = shape_system(name, nd)
        return cache[(name, nd)]
    return get


def to_hip(hip, A, I=None, R=None):
    m = hip.hecmwST_matrix.from_arrays(A.N, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, A.B.copy(),
                                       NDOF=A.NDOF)
    if I is not None:
        m.Iarray[:] = I
        m.Rarray[:] = R
    return m


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def shape_nd(names):
    return [(s, nd) for s in names for nd in SHAPE_NDOF[s]]


@pytest.mark.parametrize("shape,nd", shape_nd(("cube20", "random", "big")))
def test_matvec(hip, oracle, systems, shape, nd):
    A = systems(shape, nd)
    m = to_hip(hip, A)
    x = np.random.default_rng(nd).standard_normal(nd * A.NP)
    y = np.zeros(nd * A.NP)
    ctx = hip.SolverContext()
    hip.hecmw_matvec(None, m, x.copy(), y, ctx=ctx)
    ref = oracle.matvec(A, x)
    n = nd * A.N
    assert rel(y[:n], ref[:n]) <= 1e-13
    m.D = m.AL = m.AU = None                               # the resident values: the same bits
    y2 = np.zeros_like(y)
    hip.hecmw_matvec(None, m, x.copy(), y2, ctx=ctx)
    assert np.array_equal(y[:n], y2[:n])
    ctx.close()


def apply_cases(shape, nd):
    """(PRECOND, SIGMA_DIAG, NCOLOR_IN, iterPREmax)"""
    ncs = SSOR_NCOLOR if shape == "cube20" else (10,)
    cases = [(3, 1.0, 10, 1), (3, 1.0, 10, 2)]
    cases += [(1, 1.0, nc, 1) for nc in ncs] + [(1, 1.3, ncs[0], 1), (1, 1.0, ncs[-1], 2)]
    if nd >= 4:
        cases += [(10, 1.0, 10, 1), (10, 1.3, 10, 1), (10, 1.0, 10, 2)]
    return cases


@pytest.mark.parametrize("shape,nd", shape_nd(SMALL))
def test_precond_apply(hip, oracle, systems, shape, nd):
    from oracle.refrun import default_params
    A = systems(shape, nd)
    r = np.random.default_rng(10 + nd).standard_normal(nd * A.NP)
    r[nd * A.N:] = 0.0
    for pc, sigma, nc, ipm in apply_cases(shape, nd):
        I, R = default_params(method=1, precond=pc, ncolor=nc, sigma_diag=sigma, iterpremax=ipm)
        ctx = hip.SolverContext()
        z = ctx.nn_precond_apply(to_hip(hip, A, I, R), r)
        st = ctx.nn_precond_stats()
        P = oracle.Precond(A, pc, sigma_diag=sigma, ncolor_in=nc, nthreads=4)
        zo = P.apply(r, iterpremax=ipm)
        case = (pc, sigma, nc, ipm)
        assert st["kind"] == pc, case
        assert rel(z[:nd * A.N], zo[:nd * A.N]) <= 1e-12, case
        if pc == 1:
            rows = np.diff(P.colorindex)
            assert st["levels"] == len(rows) and st["slices"] == (-(-rows // 64)).sum(), case
        if pc == 10:
            assert st["factor_lanes"] == (32 if shape == "cube20" else 1), case
            assert st["slices"] > st["levels"] and st["dataflow"] == 1 and st["df_fallbacks"] == 0, case
            assert 1 <= st["df_grid"] <= st["slices"], case
        ctx.close()


@pytest.mark.parametrize("shape,nd", [(s, nd) for s in SMALL for nd in (4, 5, 6)])
def test_ilu_sweep_forms_bitwise(hip, oracle, systems, shape, nd):
    """The persistent dataflow sweep at the default grid, at grids that do not divide the slice count (each workgroup walks
    several slices, forward strided, backward from its last one), and the launch-per-level sweeps: the same bits, and no sweep
    timed out."""
    from oracle.refrun import default_params
    A = systems(shape, nd)
    I, R = default_params(method=1, precond=10)
    ctx = hip.SolverContext()
    z0 = ctx.nn_precond_apply(to_hip(hip, A, I, R), A.B)
    st = ctx.nn_precond_stats()
    slices = st["slices"]
    assert st["dataflow"] == 1 and st["df_fallbacks"] == 0 and st["df_grid"] <= slices
    assert rel(z0[:nd * A.N], oracle.Precond(A, 10).apply(A.B)[:nd * A.N]) <= 1e-12
    for g in (1, 2, 3, 7, slices - 1):
        ctx.set_option("FX_DF_GRID", g)
        z = ctx.nn_precond_apply(to_hip(hip, A, I, R), A.B)
        st = ctx.nn_precond_stats()
        assert st["df_grid"] == g and st["df_fallbacks"] == 0, (g, st)
        assert np.array_equal(z, z0), g
    ctx.close()
    b = hip.SolverContext()
    b.set_option("FX_DATAFLOW", 0)
    z = b.nn_precond_apply(to_hip(hip, A, I, R), A.B)
    assert b.nn_precond_stats()["dataflow"] == 0 and np.array_equal(z, z0)
    b.close()


def compare_solve(hip, oracle, A, I, R, ctx=None, hist_all=False):
    """GPU hecmw_solve against oracle.solve_iterative with the bounds of tests/test_gpu_nn.py; returns the GPU matrix."""
    meth = int(I[1])
    o = oracle.solve_iterative(A, I, R, nthreads=4)
    m = to_hip(hip, A, I, R)
    own = ctx is None
    ctx = ctx or hip.SolverContext()
    code = hip.hecmw_solve(None, m, ctx=ctx)
    n = A.NDOF * A.N
    tol_it, tol_x = (1, 1e-8) if meth <= 2 else (max(1, int(0.1 * o["iter"])), 1e-7)
    assert code == o["code"], (code, o["code"])
    assert abs(ctx.info.iterations - o["iter"]) <= tol_it, (ctx.info.iterations, o["iter"])
    if code == 0:
        assert m.Iarray[80] == 1
    assert rel(m.X[:n], o["X"][:n]) <= tol_x
    h, ho = ctx.history, o["history"]
    k = min(len(h), len(ho)) if hist_all else min(5, len(h), len(ho))
    assert k >= 1 and (not hist_all or len(h) == len(ho))
    assert np.all(np.abs(h[:k] - ho[:k]) <= 1e-7 * ho[0] + 1e-6 * ho[:k])
    if own:
        ctx.close()
    return m


def solve_cases(nd):
    return [(meth, pc) for meth in (1, 2, 3, 4) for pc in (3, 1, 10) if pc != 10 or nd >= 4]


@pytest.mark.parametrize("shape,nd", shape_nd(SMALL))
def test_solves(hip, oracle, systems, shape, nd):
    from oracle.refrun import default_params
    A = systems(shape, nd)
    for meth, pc in solve_cases(nd):
        I, R = default_params(method=meth, precond=pc)
        if nd == 6 and pc == 1:
            I[0] = 5       # the reference's SSOR_66 quirk: an unsymmetric preconditioner, compare a fixed number of steps
        compare_solve(hip, oracle, A, I, R)


@pytest.mark.parametrize("nd,meth,pc", [(1, 1, 1), (1, 2, 3), (2, 1, 1), (2, 2, 3)])
def test_big_fixed_steps(hip, oracle, systems, nd, meth, pc):
    """40 steps of CG + SSOR and BiCGSTAB + DIAG where the vector kernels loop over their grid and k_nn_reduce sums more than
    256 partials: the whole residual history and the unconverged X."""
    from oracle.refrun import default_params
    A = systems("big", nd)
    assert nd * A.N > 2048 * 256
    I, R = default_params(method=meth, precond=pc, maxit=40)
    compare_solve(hip, oracle, A, I, R, hist_all=True)


@pytest.mark.parametrize("shape,meth,pc,maxit", [("cube20", 1, 1, 10000), ("cube20", 2, 3, 10000), ("big", 1, 3, 40)])
def test_scaling_ndof1(hip, oracle, systems, shape, meth, pc, maxit):
    """SCALING=YES on scalar systems (k_nn_scale_bell's pair-packed branch); afterwards the resident matrix is unscaled."""
    from oracle.refrun import default_params
    A = systems(shape, 1)
    I, R = default_params(method=meth, precond=pc, maxit=maxit)
    I[6] = 1
    ctx = hip.SolverContext()
    m = compare_solve(hip, oracle, A, I, R, ctx=ctx, hist_all=True)
    x = np.random.default_rng(5).standard_normal(A.NP)
    m.D = m.AL = m.AU = None
    y = np.zeros(A.NP)
    hip.hecmw_matvec(None, m, x.copy(), y, ctx=ctx)
    ref = oracle.matvec(A, x)
    assert rel(y[:A.N], ref[:A.N]) <= 1e-12
    ctx.close()


ORDER_NDOF = (1, 5)


def ordering_run(path):
    """The SSOR apply and a CG + SSOR solve on cube20 for ORDER_NDOF, on a fresh context of this process's environment."""
    from frontistr_amd import hecmw as hip
    from oracle.refrun import default_params
    out = {}
    for nd in ORDER_NDOF:
        A = shape_system("cube20", nd)
        I, R = default_params(method=1, precond=1, ncolor=SSOR_NCOLOR[0])
        ctx = hip.SolverContext()
        out["z%d" % nd] = ctx.nn_precond_apply(to_hip(hip, A, I, R), A.B)
        out["ncolor%d" % nd] = ctx.nn_precond_stats()["levels"]
        m = to_hip(hip, A, I, R)
        out["code%d" % nd] = hip.hecmw_solve(None, m, ctx=ctx)
        out["iter%d" % nd] = ctx.info.iterations
        out["X%d" % nd] = m.X
        out["hist%d" % nd] = ctx.history
        ctx.close()
    np.savez(path, **out)


def test_device_ordering_equals_host_ordering(tmp_path):
    """FX_BFS_DEVICE_MIN / FX_MC_DEVICE_MIN below cube20's N: the SSOR set-up orders on the device; the apply and the solve give
    the bits of the host ordering.  Both run in fresh children (the thresholds are read when a context is created)."""
    res = {}
    for tag, env in (("host", {"FX_BFS_DEVICE_MIN": "100000000", "FX_MC_DEVICE_MIN": "100000000"}),
                     ("device", {"FX_BFS_DEVICE_MIN": "1000", "FX_MC_DEVICE_MIN": "1000"})):
        path = str(tmp_path / (tag + ".npz"))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_nn_shapes as T; T.ordering_run(%r)" % (HERE, ROOT, path)
        try:
            p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", code], env=dict(os.environ, **env),
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=660)
        except subprocess.TimeoutExpired:
            pytest.fail("%s ordering: child timed out" % tag)
        if p.returncode != 0:
            pytest.fail("%s ordering: child exited with %d\n%s" % (tag, p.returncode, p.stdout[-3000:]))
        res[tag] = dict(np.load(path))
    for nd in ORDER_NDOF:
        assert res["host"]["code%d" % nd] == 0 and res["host"]["iter%d" % nd] > 1
        for k in ("z", "ncolor", "code", "iter", "X", "hist"):
            assert np.array_equal(res["host"]["%s%d" % (k, nd)], res["device"]["%s%d" % (k, nd)]), (nd, k)
