"""The numpy restatement of block ILU(0) (tests/nn_ilu_ref.py) against the reference's own hecmw_precond_BILU_nn / _66
set-up + apply (mode 3 vectors of tests/golden/nn_ilu.npz).  CPU only: it pins the fixture and serves as the readable
specification the GPU tests also use (NDOF = 4, where the reference cannot run: see make_nn_ilu_golden.py)."""
import numpy as np
import pytest

import nn_ilu_ref
from conftest import load_golden
from nn_cases import nn_system


@pytest.mark.parametrize("nd", [5, 6])
@pytest.mark.parametrize("k", [0, 1])
def test_restatement_matches_reference(nd, k):
    g = load_golden("nn_ilu")
    A = nn_system(nd)
    z = nn_ilu_ref.apply(A, nn_ilu_ref.factor(A, float(g["sigmas"][k])), A.B)
    zr = g["z_n%d_s%d" % (nd, k)]
    assert np.abs(z - zr).max() <= 1e-13 * np.abs(zr).max()


def test_restatement_preconditioner_form():
    """A self-check of the restatement, not of the library: apply() is M^-1 for M = (D + L~) D^-1 (D + U~), with D the
    unmodified (sigma-scaled) diagonal blocks and L~, U~ the updated off-diagonal blocks factor() returns -- the form the
    reference's factors take, because its Schur update of the diagonal block never runs."""
    from oracle.refrun import BSR
    nd, n = 4, 12
    rng = np.random.default_rng(1)
    indexL = np.r_[0, np.arange(n)].astype(np.int32)
    indexU = np.r_[np.arange(n), n - 1].astype(np.int32)
    itemL = np.arange(1, n, dtype=np.int32)
    itemU = np.arange(2, n + 1, dtype=np.int32)
    D = np.array([rng.standard_normal((nd, nd)) + 8 * np.eye(nd) for _ in range(n)])
    AL = rng.standard_normal((n - 1, nd, nd))
    AU = rng.standard_normal((n - 1, nd, nd))
    A = BSR(n, n, indexL, itemL, indexU, itemU, D.ravel(), AL.ravel(), AU.ravel(), np.zeros(nd * n), NDOF=nd)
    M = np.zeros((nd * n, nd * n))
    for i in range(n):
        M[nd * i:nd * i + nd, nd * i:nd * i + nd] = D[i]
        if i > 0:
            M[nd * i:nd * i + nd, nd * (i - 1):nd * i] = AL[i - 1]
            M[nd * (i - 1):nd * i, nd * i:nd * i + nd] = AU[i - 1]
    x = rng.standard_normal(nd * n)
    F = nn_ilu_ref.factor(A)
    # the reference's Dlu is the LU of D alone, so M = (D + L~) D^-1 (D + U~) with the updated blocks
    z = nn_ilu_ref.apply(A, F, M @ x)
    Dlu, L, U = F
    Dm, Lm, Um = np.zeros_like(M), np.zeros_like(M), np.zeros_like(M)
    for i in range(n):
        Dm[nd * i:nd * i + nd, nd * i:nd * i + nd] = D[i]
        if i > 0:
            Lm[nd * i:nd * i + nd, nd * (i - 1):nd * i] = L[i - 1]
            Um[nd * (i - 1):nd * i, nd * i:nd * i + nd] = U[i - 1]
    P = (Dm + Lm) @ np.linalg.solve(Dm, Dm + Um)
    assert np.allclose(z, np.linalg.solve(P, M @ x), rtol=1e-10, atol=1e-10)
