#!/usr/bin/env python3
"""tests/golden/nn_ilu.npz: the REFERENCE's block ILU(0) (PRECOND = 10) on the synthetic NDOF = 4, 5, 6 systems of
tests/nn_cases.py -- hecmw_precond_BILU_nn / _66 through oracle/_ref/ref_solve (serial: the BILU apply is serial anyway).
NDOF = 5 and 6 only: the reference's FORM_ILU0_44 allocates Dlu0 / ALlu0 / AUlu0 with 9 values per block and writes 16
(hecmw_precond_BILU_44.f90:221), so ref_solve ends in a segmentation fault at NDOF = 4.  The tests pin NDOF = 4 against
tests/nn_ilu_ref.py, which test_nn_ilu_ref.py checks against this file at NDOF = 5 and 6.  Stored:
  z_n<nd>_s<k>      mode 3 (hecmw_precond_setup + hecmw_precond_apply): Z = M^-1 B for SIGMA_DIAG = SIGMAS[k]
  n<nd>_m<meth>_*   mode 1 solves, METHOD 1-4: iterations, ITERLOG history, X
  n6_scal_*         SCALING=YES (CG);   n5_ipm2_*: iterPREmax = 2 (BiCGSTAB)
  recycle_*         NDOF 6, CG: six solves of ref_solve mode 4 (D grows by 10 % and Iarray(97) = 1 before solves 2-6, X reset:
                    the preconditioner recycle policy of hecmw_matrix_misc.f90:678-697); iterations of every solve, last X
  retry_*           SIGMA_DIAG = -1 ('auto') on a system whose first attempt diverges: the attempt lengths of the retries

    python tests/golden/make_nn_ilu_golden.py        (needs oracle/_ref, built by oracle/build_ref.py)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nn_cases import nn_system  # noqa: E402
from oracle import refrun  # noqa: E402

SIGMAS = (1.0, 1.3)
RETRY = (5, 10, -0.05)  # (NDOF, block whose diagonal block is scaled, scale)


def retry_system():
    nd, blk, scale = RETRY
    A = nn_system(nd)
    A.D = A.D.copy()
    A.D[nd * nd * blk:nd * nd * (blk + 1)] *= scale
    return A


def attempts(history):
    lens, cur = [], 0
    for it, _ in history:
        if it == 1 and cur:
            lens.append(cur)
            cur = 0
        cur += 1
    lens.append(cur)
    return lens


def solve(out, tag, A, meth, maxit=10000, **kw):
    I, R = refrun.default_params(method=meth, precond=10, maxit=maxit)
    for k, v in kw.items():
        if k == "scaling":
            I[6] = v
        elif k == "iterpremax":
            I[4] = v
        elif k == "sigma":
            R[1] = v
    r = refrun.run_solve(A, I, R, threads=1)
    assert r["returncode"] == 0, r["stdout"][-2000:]
    out[tag + "iter"] = np.int32(r["iter"])
    out[tag + "hist"] = np.array([h[1] for h in r["history"]])
    out[tag + "X"] = r["X"]
    out[tag + "attempts"] = np.array(attempts(r["history"]), dtype=np.int32)
    out[tag + "Iarray"] = r["Iarray"]
    out[tag + "n_attempts"] = np.int32(1 + sum("Increasing SIGMA_DIAG" in ln for ln in r["stdout"].splitlines()))
    print(tag, "iter", r["iter"], "attempts", attempts(r["history"]), "I81/82", r["Iarray"][80], r["Iarray"][81])


def main():
    out = {}
    for nd in (5, 6):
        A = nn_system(nd)
        for k, sg in enumerate(SIGMAS):
            I, R = refrun.default_params(method=1, precond=10)
            R[1] = sg
            r = refrun.run_solve(A, I, R, mode=3, threads=1)
            assert r["returncode"] == 0, r["stdout"][-2000:]
            out["z_n%d_s%d" % (nd, k)] = r["X"]
        for meth in (1, 2, 3, 4):
            solve(out, "n%d_m%d_" % (nd, meth), A, meth)
    solve(out, "n6_scal_", nn_system(6), 1, scaling=1)
    solve(out, "n5_ipm2_", nn_system(5), 2, iterpremax=2)
    solve(out, "retry_", retry_system(), 1, maxit=500, sigma=-1.0)
    I, R = refrun.default_params(method=1, precond=10)
    r = refrun.run_solve(nn_system(6), I, R, threads=1, mode=4, nrepeat=6)
    assert r["returncode"] == 0, r["stdout"][-2000:]
    out["recycle_iters"] = np.array(r["iters"], dtype=np.int32)
    out["recycle_X"] = r["X"]
    print("recycle", r["iters"])
    out["sigmas"] = np.array(SIGMAS)
    out["retry_case"] = np.array(RETRY, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "nn_ilu.npz"), **out)


if __name__ == "__main__":
    main()
