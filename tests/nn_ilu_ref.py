"""A numpy restatement of the reference's block ILU(0) (FORM_ILU0_44 / _nn / _66 and the BILU apply routines), for the
tests.  A: an oracle.refrun.BSR with NDOF = nd.  Readable, not fast: rows in natural order as the reference walks them."""
import numpy as np


def _lu(a):
    """ILU1a: LU without pivoting, reciprocal pivots on the diagonal."""
    a = a.copy()
    n = a.shape[0]
    for k in range(n):
        a[k, k] = 1.0 / a[k, k]
        for i in range(k + 1, n):
            a[i, k] = a[i, k] * a[k, k]
            for j in range(k + 1, n):
                a[i, j] = a[i, j] - a[i, k] * a[k, j]
    return a


def _solve(lu, x):
    """The triangular solves of ILU1b and of the apply (forward, then backward with the reciprocal pivots)."""
    x = x.copy()
    n = lu.shape[0]
    for i in range(1, n):
        for j in range(i):
            x[i] = x[i] - lu[i, j] * x[j]
    for i in range(n - 1, -1, -1):
        for j in range(n - 1, i, -1):
            x[i] = x[i] - lu[i, j] * x[j]
        x[i] = lu[i, i] * x[i]
    return x


def factor(A, sigma_diag=1.0):
    """(Dlu, AL, AU) of rows 0..N-1: Dlu = LU of the sigma-scaled diagonal blocks (the Schur update of the diagonal never
    runs), AL / AU the updated off-diagonal blocks.  Halo columns are left as they are (they multiply ZP(halo) = 0)."""
    nd, N = A.NDOF, A.N
    D = A.D.reshape(-1, nd, nd)[:N].copy()
    D[:, np.arange(nd), np.arange(nd)] *= sigma_diag
    Dlu = np.array([_lu(d) for d in D])
    AL = A.AL.reshape(-1, nd, nd).copy()
    AU = A.AU.reshape(-1, nd, nd).copy()
    iL, jL, iU, jU = A.indexL, A.itemL - 1, A.indexU, A.itemU - 1
    for i in range(1, N):
        posL = {int(jL[p]): p for p in range(iL[i], iL[i + 1])}
        posU = {int(jU[p]): p for p in range(iU[i], iU[i + 1])}
        for kk in range(iL[i], iL[i + 1]):
            k = int(jL[kk])
            aik = AL[kk].copy()
            for jj in range(iU[k], iU[k + 1]):
                j = int(jU[jj])
                if j >= N or (j not in posL and j not in posU):
                    continue
                x = np.array([_solve(Dlu[k], AU[jj][:, c]) for c in range(nd)]).T   # Dk^-1 Akj, column by column
                rhs = np.zeros((nd, nd))
                for r in range(nd):
                    for c in range(nd):
                        s = aik[r, 0] * x[0, c]
                        for q in range(1, nd):
                            s = s + aik[r, q] * x[q, c]
                        rhs[r, c] = s
                if j < i:
                    AL[posL[j]] -= rhs
                else:
                    AU[posU[j]] -= rhs
    return Dlu, AL, AU


def apply(A, F, r):
    """z = M^-1 r (hecmw_precond_BILU_nn_apply with ZP(halo) = 0); r, z: NDOF * NP, z's halo part 0."""
    Dlu, AL, AU = F
    nd, N = A.NDOF, A.N
    w = np.zeros(nd * A.NP)
    w[:nd * N] = r[:nd * N]
    iL, jL, iU, jU = A.indexL, A.itemL - 1, A.indexU, A.itemU - 1
    for i in range(N):
        sw = w[nd * i:nd * i + nd].copy()
        for p in range(iL[i], iL[i + 1]):
            k = jL[p]
            sw -= AL[p] @ w[nd * k:nd * k + nd]
        w[nd * i:nd * i + nd] = _solve(Dlu[i], sw)
    for i in range(N - 1, -1, -1):
        sw = np.zeros(nd)
        for p in range(iU[i + 1] - 1, iU[i] - 1, -1):
            k = jU[p]
            sw += AU[p] @ w[nd * k:nd * k + nd]
        w[nd * i:nd * i + nd] -= _solve(Dlu[i], sw)
    return w
