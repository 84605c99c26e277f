"""The shapes of tests/test_gpu_nn_shapes.py reach the cases they are there for, computed from the profile alone (the oracle's
colour index, a copy of the device level schedule, the slice widths), so a shape that drifts off its case fails on every
machine, not only on one with a GPU.  And the vectorised builder is the small one at its size."""
import numpy as np
import pytest

from nn_cases import BIG_M, SSOR_NCOLOR, cube_system, ilu_levels, nn_system, random_system, spmv_widths, ssor_layout


@pytest.mark.parametrize("nd", [1, 2, 4, 5, 6])
def test_cube_system_is_nn_system(nd):
    A, B = nn_system(nd), cube_system(nd, 4)
    for k in ("indexL", "itemL", "indexU", "itemU", "D", "AL", "AU", "B"):
        assert np.array_equal(getattr(A, k), getattr(B, k)), k
    H = cube_system(nd, 4, halo=7)
    assert H.NP == A.NP and H.N == A.NP - 7 and np.array_equal(H.AU, A.AU)


def pair_cases(widths):
    """The three cases of the NDOF = 1 pair-packed row loop of k_nn_rows: two pairs at a time, a leftover pair, an odd entry."""
    w = np.asarray(widths)
    return {"two_pairs": bool(((w >> 1) >= 2).any()), "leftover_pair": bool(((w >> 1) & 1).any()), "odd_entry": bool((w & 1).any())}


def test_cube20_reaches_the_multi_slice_cases(oracle):
    A = cube_system(1, 20)
    assert A.N == 9261 and A.N % 64 == 45
    w = spmv_widths(A)
    assert len(w) % 4 == 1 and all(pair_cases(w).values())           # SpMV: a partly filled last workgroup, all three pair cases
    got = {}
    for nc in SSOR_NCOLOR:
        P = oracle.Precond(A, 1, ncolor_in=nc, nthreads=4)
        rows = np.diff(P.colorindex)
        assert rows.sum() == A.N
        for lower in (True, False):
            sl, wid = ssor_layout(A, P.perm, P.colorindex, lower)
            assert np.array_equal(sl, -(-rows // 64))
            got["colour_over_4_slices"] = got.get("colour_over_4_slices", False) or bool((sl > 4).any())
            got["partial_last_workgroup"] = got.get("partial_last_workgroup", False) or bool(((sl > 4) & (sl % 4 != 0)).any())
            for k, v in pair_cases(wid).items():
                got[k] = got.get(k, False) or v
        got["rows_1_mod_64"] = got.get("rows_1_mod_64", False) or bool((rows % 64 == 1).any())
        got["rows_63_mod_64"] = got.get("rows_63_mod_64", False) or bool((rows % 64 == 63).any())
    assert all(got.values()), got
    _, cnt = ilu_levels(A)
    slices = -(-cnt // 64)
    assert len(cnt) == 141 and (cnt > 64).sum() == 77 and slices.sum() == 218
    assert slices.sum() < 256          # fewer slices than CUs: only FX_DF_GRID makes a dataflow workgroup own several
    nblk = np.diff(A.indexL) + np.diff(A.indexU)
    assert nblk.max() <= 32            # the 32-lanes-per-row factor, levels of up to 116 rows: 15 of its workgroups
    assert cnt.max() > 8 * 8


def test_random_reaches_halo_hub_isolated_and_wide_levels():
    for nd in (1, 4):                  # the profile does not depend on NDOF
        A = random_system(nd, 3000, 40, 7, general=True)
        assert A.NP > A.N and (A.itemU > A.N).any()                    # halo columns, dropped by the ILU symbolic phase
        nblk = np.diff(A.indexL)[:A.N] + np.diff(A.indexU)[:A.N]
        assert (nblk == 0).any() and nblk.max() > 32                   # isolated rows; a hub row: the one-thread factor
        _, cnt = ilu_levels(A)
        assert (cnt > 128).sum() >= 11                                 # levels over one k_nn_ilu0_factor_level workgroup
        AL = A.AL.reshape(-1, nd, nd)
        if nd > 1:
            assert not np.allclose(AL, AL.transpose(0, 2, 1))          # a transposed block is visible


def test_big_runs_the_grid_stride_loops():
    """NDOF * N > 2048 blocks x 256 threads: the Krylov vector kernels loop, and k_nn_reduce sums more than 256 partials. From the
    sizes alone (the matrices are built by the GPU module only)."""
    for nd, m in BIG_M.items():
        N = (m + 1) ** 3
        assert nd * N > 2048 * 256
