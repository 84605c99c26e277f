"""Block ILU(0) (PRECOND = 10) of the CPU oracle for NDOF = 4, 5, 6 (oracle/hecmw_nn_oracle.c: FORM_ILU0_nn / _44 / _66 and the
BILU apply) against the vectors the REAL reference produced (tests/golden/nn_ilu.npz, NDOF 5 and 6), and against the numpy
restatement tests/nn_ilu_ref.py where the reference has no run (NDOF 4: its BILU_44 overruns its arrays) or at wide rows."""
import numpy as np
import pytest

import nn_ilu_ref
from conftest import load_golden
from nn_cases import nn_system, random_system, wide_system


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("nd", [5, 6])
def test_oracle_ilu_apply_bit_identical_to_reference(oracle, nd):
    g = load_golden("nn_ilu")
    A = nn_system(nd)
    for k, sigma in enumerate(g["sigmas"]):
        z = oracle.Precond(A, 10, sigma_diag=float(sigma)).apply(A.B)
        assert np.array_equal(z, g["z_n%d_s%d" % (nd, k)]), (nd, sigma)


def solve_case(oracle, A, meth, maxit=10000, **kw):
    from oracle.refrun import default_params
    I, R = default_params(method=meth, precond=10, maxit=maxit)
    I[6], I[4] = kw.get("scaling", 0), kw.get("iterpremax", 1)
    if "sigma" in kw:
        R[1] = kw["sigma"]
    return oracle.solve_iterative(A, I, R, nthreads=1)


def check_solve(o, g, tag, flag=True):
    """flag: Iarray(81) too (the SCALING run of the reference leaves it 0 after converging, which the oracle does not copy)."""
    assert o["code"] == 0 and o["iter"] == int(g[tag + "iter"]), tag
    assert not flag or o["Iarray"][80] == g[tag + "Iarray"][80] == 1, tag
    assert np.array_equal(o["X"], g[tag + "X"]), tag
    hr = g[tag + "hist"]
    n = min(len(o["history"]), len(hr))
    assert n == int(g[tag + "iter"]) and np.all(np.abs(o["history"][:n] - hr[:n]) <= 1e-6 * hr[:n])   # stdout prints 7 digits


@pytest.mark.parametrize("nd", [5, 6])
@pytest.mark.parametrize("meth", [1, 2, 3, 4])
def test_oracle_ilu_solve_bit_identical_to_reference(oracle, nd, meth):
    tag = "n%d_m%d_" % (nd, meth)
    check_solve(solve_case(oracle, nn_system(nd), meth), load_golden("nn_ilu"), tag)


def test_oracle_ilu_scaling_and_iterpremax_bit_identical_to_reference(oracle):
    g = load_golden("nn_ilu")
    check_solve(solve_case(oracle, nn_system(6), 1, scaling=1), g, "n6_scal_", flag=False)
    check_solve(solve_case(oracle, nn_system(5), 2, iterpremax=2), g, "n5_ipm2_")


def test_oracle_ilu_sigma_retry_and_recycle_match_reference(oracle):
    """SIGMA_DIAG = -1 on a system whose first attempt diverges (the retries keep the first attempt's factors), and six solves
    under the recycle policy at NDOF 6 (BILU_66 factors again on every set-up, flags or not): the reference's counts and X."""
    from oracle.refrun import default_params
    g = load_golden("nn_ilu")
    nd, blk, scale = g["retry_case"]
    nd, blk = int(nd), int(blk)
    A = nn_system(nd)
    A.D = A.D.copy()
    A.D[nd * nd * blk:nd * nd * (blk + 1)] *= scale
    o = solve_case(oracle, A, 1, maxit=500, sigma=-1.0)
    assert o["iter"] == int(g["retry_iter"]) and o["Iarray"][80] == g["retry_Iarray"][80]
    assert np.array_equal(o["X"], g["retry_X"])
    I, R = default_params(method=1, precond=10)
    iters, X, _ = oracle.solve_sequence(nn_system(6), I, R, 6)
    assert iters == list(g["recycle_iters"]) and np.array_equal(X, g["recycle_X"])


@pytest.mark.parametrize("make", [lambda nd: nn_system(nd), wide_system, lambda nd: random_system(nd, 300, 20, 11, general=True)],
                         ids=["cube", "wide", "random_halo"])
@pytest.mark.parametrize("nd", [4, 5, 6])
@pytest.mark.parametrize("sigma", [1.0, 1.3])
def test_oracle_ilu_matches_numpy_restatement(oracle, make, nd, sigma):
    """NDOF 4 has no reference run; wide rows (> 32 blocks) and halo columns (NP > N) have none either: the numpy restatement
    is the anchor, to 1e-14 relative (it sums in a different order only inside the column solves)."""
    A = make(nd)
    z = oracle.Precond(A, 10, sigma_diag=sigma).apply(A.B)
    zr = nn_ilu_ref.apply(A, nn_ilu_ref.factor(A, sigma), A.B)
    assert np.all(z[nd * A.N:] == 0.0)
    assert rel(z[:nd * A.N], zr[:nd * A.N]) <= 1e-14


def test_oracle_ilu_of_other_block_sizes_is_refused(oracle):
    for nd in (1, 2):
        with pytest.raises(ValueError):
            oracle.Precond(nn_system(nd), 10)
