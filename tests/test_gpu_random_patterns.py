"""Profiles that do not come from a mesh: random symmetric sparsity with isolated nodes (rows holding only their diagonal
block), a hub row (more than 32 off-diagonal blocks: the wide-row kernels), very uneven row lengths (slice padding) and halo
columns without a communicator.  SPD block values: sum over edges of [[P, -P], [-P, P]] with P SPD, plus a diagonal shift.
GPU against the CPU oracle for the 3x3 path (all preconditioners) and the generic-block path."""
import numpy as np
import pytest

from nn_cases import random_system

pytestmark = pytest.mark.gpu


def to_hip(hip, A):
    return hip.hecmwST_matrix.from_arrays(A.N, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU, A.B.copy(),
                                          NDOF=A.NDOF)


@pytest.mark.parametrize("nd,N,n_halo,seed", [(3, 300, 0, 1), (3, 517, 40, 2), (3, 64, 0, 3), (2, 300, 25, 4), (6, 130, 0, 5),
                                              (1, 1000, 0, 6)])
def test_random_pattern_matvec_and_solves(hip, oracle, nd, N, n_halo, seed):
    from oracle.refrun import default_params
    A = random_system(nd, N, n_halo, seed)
    ctx = hip.SolverContext()
    m = to_hip(hip, A)
    x = np.random.default_rng(seed).standard_normal(nd * A.NP)
    y = np.zeros(nd * A.NP)
    hip.hecmw_matvec(None, m, x.copy(), y, ctx=ctx)
    ref = oracle.matvec(A, x)
    assert np.abs(y[:nd * N] - ref[:nd * N]).max() <= 1e-13 * np.abs(ref).max()
    cases = [(1, 3), (1, 1), (2, 1)] + ([(2, 10), (1, 10), (3, 3), (4, 1)] if nd == 3 else [])
    for meth, pc in cases:
        I, R = default_params(method=meth, precond=pc)
        stagnates = (nd == 6 and meth == 1 and pc == 1)
        if stagnates:       # the reference's SSOR_66 quirk makes this preconditioner unsymmetric: its own CG stalls at 7e-5 here
            I[0] = 30
        o = oracle.solve_iterative(A, I, R, nthreads=4)
        m = to_hip(hip, A)
        m.Iarray[:] = I
        m.Rarray[:] = R
        code = hip.hecmw_solve(None, m, ctx=ctx)
        if stagnates:
            assert code == o["code"] == 3001 and m.Iarray[80] == 0 and ctx.info.iterations == o["iter"] == 31
            assert np.all(np.abs(ctx.history[:12] - o["history"][:12]) <= 1e-6 * o["history"][:12])
            continue
        assert code == o["code"] == 0 and m.Iarray[80] == 1, (meth, pc, code, o["code"])
        tol_it = max(1, int(0.15 * o["iter"])) if meth != 1 else 1
        assert abs(ctx.info.iterations - o["iter"]) <= tol_it, (meth, pc, ctx.info.iterations, o["iter"])
        assert np.abs(m.X - o["X"])[:nd * N].max() <= 2e-7 * np.abs(o["X"]).max(), (meth, pc)
    ctx.close()
