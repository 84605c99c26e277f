"""Every selectable SpMV and sweep kernel variant against the fp64 oracle.

The parity suite (test_gpu_parity.py) pins the DEFAULT kernels to the oracle.  The library ships more: each FX_* switch below
picks another kernel or data path, from the environment at fx_create or through fx_set_option on a live context, and the A/B
measurements of DESIGN.md rest on them computing the same answer.  Here every value of every such switch runs at least once with
each kernel family it affects, on shapes whose colours reach the tails of the slice loops, against the oracle with the tolerance
policy of test_gpu_parity.py (SpMV 1e-13, preconditioner apply 1e-12, solves: history lines 1-10 1e-10, CG count +-1, field 1e-9 /
BiCGSTAB 5e-8).  The switches are set in the environment before SolverContext() (or with set_option before the first upload); a
solve captures its graph again at its begin, so nothing here depends on a replay picking a switch up.

Pairs that are bit-identical by construction, asserted with np.array_equal besides the oracle bound:
  * FX_SPMV_BS 64 / 256 and FX_SPMV_SPATIAL 0 / 1: the same row loop per slice, only the slice -> workgroup map changes;
  * k_ssor_color with FX_SSOR_BS 64 / 256 and FX_SSOR_SPW 1 / 3 / 8 (same FX_PIPE_SSOR): the same row loop per slice, only which
    wave runs which slice changes (z only: the r.z partials are grouped per workgroup, so solves differ by rounding);
  * FX_SSOR_MODE 0 / 1 for one sweep kernel: the same sweep layouts, the Krylov vectors only addressed through slot_node or not;
  * the wave-split colour / level sweeps with W waves and the dataflow launch with W waves (FX_DATAFLOW, FX_DF_SOA, FX_DF_POLL,
    FX_DF_SLEEP, FX_DF_PRESLEEP): the same bell_dot3 contraction in the same order, the layout and waiting are all that differ.
Not bit-identical (rounding differs, only the oracle bound is claimed): FX_PIPE_SPMV / FX_PIPE_SSOR (two code shapes of the row
loop), split against non-split sweeps (bell_dot3 against bell_row_sweep), different FX_SPLIT_WPS, and the Eisenstat switches.
"""
import numpy as np
import pytest

from test_gpu_parity import check_solve, relerr, to_hecmat
from test_gpu_random_patterns import random_system

pytestmark = pytest.mark.gpu

SIGMA = 1.3            # SIGMA_DIAG of the multicolour SSOR cases: exercises the (D - D~) terms of Eisenstat's form
CUBE_N = 26            # 27^3 = 19,683 rows
# name -> ncolor_in (Iarray[33]) of the cube; "hub" is the random pattern
SHAPES = {"cube_c4": 4, "cube_c10": 10, "cube_c37": 37, "hub": 10}
CUBES = ["cube_c4", "cube_c10", "cube_c37"]
VARIANT_ENV = ("FX_PIPE_SPMV", "FX_SPMV_BS", "FX_SPMV_SPATIAL", "FX_SSOR_MODE", "FX_SPLIT_MAX_SLICES", "FX_SSOR_BS", "FX_PIPE_SSOR",
               "FX_SSOR_SPW", "FX_PIPE_MAX_SLICES", "FX_SPLIT_WPS", "FX_DATAFLOW", "FX_DF_SOA", "FX_DF_SLEEP", "FX_DF_PRESLEEP",
               "FX_DF_POLL", "FX_DF_WPS", "FX_EISENSTAT", "FX_EIS_FUSE", "FX_EIS_MERGE", "FX_EIS_GRID", "FX_SSOR_NATURAL",
               "FX_LAYOUT_DEVICE")


class Shape:
    def __init__(self, name, A, ncolor_in):
        self.name, self.A, self.ncolor_in = name, A, ncolor_in
        self.x = np.sin(0.37 * np.arange(3 * A.NP) + 0.1)
        self.r = np.cos(0.11 * np.arange(3 * A.NP) + 0.3)
        self._cache = {}

    def once(self, key, f):
        if key not in self._cache:
            self._cache[key] = f()
        return self._cache[key]

    def params(self, meth, pc, sigma=1.0):
        from oracle.refrun import default_params
        return default_params(method=meth, precond=pc, sigma_diag=sigma, ncolor=self.ncolor_in)

    def slices(self, oracle):
        """Rows and 64-row slices per colour of the reference's multicolour ordering (what the GPU sweeps launch per colour)."""
        def f():
            ci = oracle.Precond(self.A, 1, sigma_diag=SIGMA, ncolor_in=self.ncolor_in, nthreads=4).colorindex
            rows = np.diff(ci)
            return rows, (rows + 63) // 64
        return self.once("slices", f)


@pytest.fixture(scope="module")
def shapes(oracle):
    from frontistr_amd.mesh import CubeMesh
    mesh = CubeMesh(CUBE_N, skew=0.03)
    A = oracle.assemble(1, mesh.coord, mesh.conn, 210000.0, 0.3, bc=mesh.dirichlet(), load=mesh.load())
    out = {k: Shape(k, A, nc) for k, nc in SHAPES.items() if k != "hub"}
    # halo columns (NP > N), a hub row of more than 32 blocks (wide-row kernels) and one of more than FX_BELL_MAXROW = 160 (the
    # device layout builder hands the whole layout to the host builder)
    out["hub"] = Shape("hub", random_system(3, 900, 16, 11, hub=(40, 200)), SHAPES["hub"])
    return out


def tail_cases(rows, sl):
    """The slice-loop tails a set of colours reaches: a one-slice colour, row counts 1 and 63 mod 64, and slice counts 1 and spb-1
    mod spb for the slices-per-workgroup spb = (FX_SSOR_BS / 64) * FX_SSOR_SPW in {4, 8, 32} (spb = 1: every colour)."""
    got = {"one_slice": bool((sl == 1).any()), "rows_1_mod_64": bool((rows % 64 == 1).any()),
           "rows_63_mod_64": bool((rows % 64 == 63).any())}
    for spb in (4, 8, 32):
        got["slices_1_mod_%d" % spb] = bool((sl % spb == 1).any())
        got["slices_%d_mod_%d" % (spb - 1, spb)] = bool((sl % spb == spb - 1).any())
    return got


def test_shapes_reach_the_tail_cases(shapes, oracle):
    """cube_c10: one-slice colours, 63 rows mod 64, slices 1 mod 4 / 8 / 32 and 31 mod 32 (eight colours of 31 slices);
    cube_c37: 1 row mod 64; cube_c4: eight big colours (35-43 slices) only; hub: halo columns and two hub rows (> 32, > 160 blocks).
    Computed from the oracle's colour index, so changing a shape so that a case is lost fails here."""
    union = {}
    for k in CUBES:
        rows, sl = shapes[k].slices(oracle)
        assert rows.sum() == shapes[k].A.N
        for case, hit in tail_cases(rows, sl).items():
            union[case] = union.get(case, False) or hit
    assert all(union.values()), union
    rows, sl = shapes["cube_c4"].slices(oracle)
    assert sl.min() > 32 and len(sl) == 8                        # big colours only: many 4- / 8-slice workgroups per colour
    A = shapes["hub"].A
    nblk = 1 + np.diff(A.indexL) + np.diff(A.indexU)
    assert A.NP > A.N and nblk[:A.N].max() > 160 and ((nblk[:A.N] > 32) & (nblk[:A.N] <= 160)).any()


def fresh_ctx(hip, monkeypatch, env):
    for k in VARIANT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return hip.SolverContext()


def tag_of(env):
    return ",".join("%s=%s" % (k[3:], v) for k, v in env.items()) or "defaults"


# ------------------------------------------------------------------------------------------------------------------------
# SpMV: FX_PIPE_SPMV x FX_SPMV_BS x FX_SPMV_SPATIAL, in the natural (FX_SSOR_MODE=0) and colour-major (1) numbering
# ------------------------------------------------------------------------------------------------------------------------
SPMV_VARIANTS = [dict(FX_PIPE_SPMV=p, FX_SPMV_BS=bs, FX_SPMV_SPATIAL=sp) for p in (1, 0) for bs in (256, 64) for sp in (1, 0)]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", [1, 0])
def test_spmv_variants(hip, oracle, shapes, shape, mode, monkeypatch):
    """hecmw_matvec after the multicolour SSOR set-up (which puts the solver into its numbering) against oracle.matvec; the four
    (FX_SPMV_BS, FX_SPMV_SPATIAL) layouts of one FX_PIPE_SPMV give the same bits."""
    S = shapes[shape]
    yo = S.once("matvec", lambda: oracle.matvec(S.A, S.x))
    out = {}
    for env in SPMV_VARIANTS:
        ctx = fresh_ctx(hip, monkeypatch, dict(env, FX_SSOR_MODE=mode))
        m = to_hecmat(hip, S.A)
        m.Iarray[2] = 1; m.Iarray[33] = S.ncolor_in
        ctx.upload(m)
        ctx.precond_setup(m)
        y = np.zeros(3 * S.A.NP)
        hip.hecmw_matvec(None, m, S.x.copy(), y, ctx=ctx)
        ctx.close()
        assert relerr(y[:3 * S.A.N], yo[:3 * S.A.N]) < 1e-13, tag_of(env)
        out[tag_of(env)] = y[:3 * S.A.N]
        ref = out[tag_of(dict(env, FX_SPMV_BS=256, FX_SPMV_SPATIAL=1))]
        assert np.array_equal(y[:3 * S.A.N], ref), tag_of(env)


@pytest.mark.parametrize("env", SPMV_VARIANTS, ids=tag_of)
def test_spmv_variants_in_cg_diag(hip, oracle, shapes, env, monkeypatch):
    """The SpMV variants inside the CG loop (block-Jacobi: natural numbering) against the oracle's solve."""
    S = shapes["cube_c10"]
    I, R = S.params(1, 3)
    o = S.once("cg_diag", lambda: oracle.solve_iterative(S.A, I, R, nthreads=4))
    ctx = fresh_ctx(hip, monkeypatch, env)
    m = to_hecmat(hip, S.A)
    m.Iarray[:] = I; m.Rarray[:] = R
    assert hip.hecmw_solve(None, m, ctx=ctx) == 0
    check_solve(ctx.info, ctx.history, m.X, o["iter"], o["history"], o["X"], 1, printed=False)
    ctx.close()


def test_device_and_host_layouts_of_the_hub_system(hip, oracle, shapes, monkeypatch):
    """A row of more than FX_BELL_MAXROW blocks: the device layout builder falls back to the host builder for the whole layout.
    FX_LAYOUT_DEVICE 1 / 0 then give identical layouts (pair / block counts) and the same bits in the product, the SSOR apply and
    the ILU(0) apply -- and both match the oracle."""
    S = shapes["hub"]
    yo = S.once("matvec", lambda: oracle.matvec(S.A, S.x))
    out = {}
    for dev in (1, 0):
        res = []
        for pc in (1, 10):
            ctx = fresh_ctx(hip, monkeypatch, dict(FX_LAYOUT_DEVICE=dev))
            m = to_hecmat(hip, S.A)
            m.Iarray[2] = pc; m.Iarray[33] = S.ncolor_in; m.Rarray[1] = SIGMA
            y = np.zeros(3 * S.A.NP)
            hip.hecmw_matvec(None, m, S.x.copy(), y, ctx=ctx)
            ctx.upload(m)
            ctx.precond_setup(m)
            z = ctx.precond_apply(S.r)
            st = ctx.stats()
            ctx.close()
            zo = oracle.Precond(S.A, pc, sigma_diag=SIGMA, ncolor_in=S.ncolor_in, nthreads=4).apply(S.r)
            assert relerr(y[:3 * S.A.N], yo[:3 * S.A.N]) < 1e-13 and relerr(z[:3 * S.A.N], zo[:3 * S.A.N]) < 1e-12, (dev, pc)
            res.append((y, z, tuple(st[k] for k in ("M_pairs", "M_blocks", "L_pairs", "L_blocks", "U_pairs", "U_blocks"))))
        out[dev] = res
    for a, b in zip(out[1], out[0]):
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------------
# multicolour SSOR apply (pc = 1)
# ------------------------------------------------------------------------------------------------------------------------
NONSPLIT = dict(FX_SPLIT_MAX_SLICES=0)


def ssor_apply_variants(mid):
    """(env, bit-group): variants of one bit-group must give the same z.  `mid`: a slice count between the colours' sizes."""
    v = []
    for wps in (0, 2, 4, 8):                                        # wave-split sweeps (the default), waves per slice
        env = dict(FX_SPLIT_WPS=wps) if wps else {}
        v.append((env, "split%d" % (wps or 4)))
        v.append((dict(env, FX_SSOR_MODE=0), "split%d" % (wps or 4)))
    for pipe in (1, 0):                                             # k_ssor_color
        for bs in (64, 256):
            for spw in (1, 3, 8):
                v.append((dict(NONSPLIT, FX_PIPE_SSOR=pipe, FX_SSOR_BS=bs, FX_SSOR_SPW=spw), "color_pipe%d" % pipe))
        v.append((dict(NONSPLIT, FX_PIPE_SSOR=pipe, FX_SSOR_BS=64, FX_SSOR_SPW=3, FX_SSOR_MODE=0), "color_pipe%d" % pipe))
    # FX_PIPE_MAX_SLICES between two colour sizes: one apply runs both row loops (no bit-group: rounding of both)
    v.append((dict(NONSPLIT, FX_PIPE_MAX_SLICES=mid, FX_SSOR_BS=256, FX_SSOR_SPW=3), None))
    v.append((dict(NONSPLIT, FX_PIPE_MAX_SLICES=mid, FX_SSOR_MODE=0), None))
    # FX_SPLIT_MAX_SLICES between two colour sizes: small colours wave-split, big ones k_ssor_color
    v.append((dict(FX_SPLIT_MAX_SLICES=mid, FX_SSOR_BS=64, FX_SSOR_SPW=8), None))
    for soa in (1, 0):                                              # one dataflow launch per apply, private sweep vectors
        v.append((dict(FX_DATAFLOW=2, FX_DF_SOA=soa, FX_SSOR_MODE=0), "split8"))
    v.append((dict(FX_DATAFLOW=2, FX_DF_WPS=4, FX_SSOR_MODE=0), "split4"))
    return v


def mid_slices(sl):
    """A slice count with colours on both sides of it (None: all colours have the same size)."""
    lo, hi = int(sl.min()), int(sl.max())
    return (lo + hi) // 2 if hi > lo else None


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ssor_apply_variants(hip, oracle, shapes, shape, monkeypatch):
    S = shapes[shape]
    zo = S.once("ssor", lambda: oracle.Precond(S.A, 1, sigma_diag=SIGMA, ncolor_in=S.ncolor_in, nthreads=4).apply(S.r))
    rows, sl = S.slices(oracle)
    mid = mid_slices(sl)
    assert mid is not None and (sl <= mid).any() and (sl > mid).any()
    groups = {}
    for env, grp in ssor_apply_variants(mid):
        ctx = fresh_ctx(hip, monkeypatch, env)
        m = to_hecmat(hip, S.A)
        m.Iarray[2] = 1; m.Iarray[33] = S.ncolor_in; m.Rarray[1] = SIGMA
        ctx.upload(m)
        ctx.precond_setup(m)
        z = ctx.precond_apply(S.r)
        z2 = ctx.precond_apply(S.r)
        st = ctx.stats()
        ctx.close()
        assert st["ncolor"] == len(sl)
        assert np.array_equal(z, z2), tag_of(env)
        assert relerr(z[:3 * S.A.N], zo[:3 * S.A.N]) < 1e-12, tag_of(env)
        if grp is not None:
            ref = groups.setdefault(grp, z[:3 * S.A.N])
            assert np.array_equal(z[:3 * S.A.N], ref), (grp, tag_of(env))


# ------------------------------------------------------------------------------------------------------------------------
# CG + multicolour SSOR solves: the fused r.z partials of the sweeps, standard loop and Eisenstat's form
# ------------------------------------------------------------------------------------------------------------------------
CG_SSOR_VARIANTS = [
    # standard loop (hecmw_solve_CG as written)
    dict(FX_EISENSTAT=0),
    dict(FX_EISENSTAT=0, FX_SPLIT_WPS=8),
    dict(FX_EISENSTAT=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=64, FX_SSOR_SPW=3),
    dict(FX_EISENSTAT=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_SSOR_SPW=8),
    dict(FX_EISENSTAT=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_PIPE_SSOR=0),
    # FX_SSOR_MODE=0: natural-order Krylov vectors -- Eisenstat's form is not taken, whatever is asked for
    dict(FX_EISENSTAT=1, FX_SSOR_MODE=0),
    dict(FX_EISENSTAT=0, FX_SSOR_MODE=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_SSOR_SPW=3),
    # Eisenstat's form: wave-split sweeps (FX_EIS_GRID: workgroups walk slices b, b + grid, ...)
    dict(FX_EISENSTAT=1),
    dict(FX_EISENSTAT=1, FX_EIS_FUSE=0, FX_EIS_MERGE=1, FX_EIS_GRID=1),
    dict(FX_EISENSTAT=1, FX_EIS_FUSE=1, FX_EIS_MERGE=0, FX_EIS_GRID=3),
    dict(FX_EISENSTAT=1, FX_EIS_FUSE=0, FX_EIS_MERGE=0, FX_EIS_GRID=0),
    dict(FX_EISENSTAT=1, FX_EIS_FUSE=1, FX_EIS_MERGE=1, FX_EIS_GRID=1),
    dict(FX_EISENSTAT=1, FX_EIS_FUSE=0, FX_EIS_MERGE=1, FX_EIS_GRID=3),
    # Eisenstat's form: k_eis_forward / k_eis_backward (non-split), both block sizes, several slices per wave
    dict(FX_EISENSTAT=1, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=64, FX_EIS_FUSE=1, FX_EIS_MERGE=1),
    dict(FX_EISENSTAT=1, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=64, FX_EIS_FUSE=0, FX_EIS_MERGE=0, FX_SSOR_SPW=3),
    dict(FX_EISENSTAT=1, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_EIS_FUSE=1, FX_EIS_MERGE=0, FX_SSOR_SPW=8),
    dict(FX_EISENSTAT=1, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_EIS_FUSE=0, FX_EIS_MERGE=1),
    # mixed: big colours k_eis_*, small ones wave-split with a grid
    dict(FX_EISENSTAT=1, FX_SPLIT_MAX_SLICES=12, FX_SSOR_BS=256, FX_EIS_GRID=3),
]


@pytest.mark.parametrize("shape", CUBES)
def test_cg_ssor_solve_variants(hip, oracle, shapes, shape, monkeypatch):
    S = shapes[shape]
    I, R = S.params(1, 1, SIGMA)
    o = S.once("cg_ssor", lambda: oracle.solve_iterative(S.A, I, R, nthreads=4))
    for env in CG_SSOR_VARIANTS:
        ctx = fresh_ctx(hip, monkeypatch, env)
        m = to_hecmat(hip, S.A)
        m.Iarray[:] = I; m.Rarray[:] = R
        code = hip.hecmw_solve(None, m, ctx=ctx)
        assert code == 0 and m.Iarray[80] == 1, (tag_of(env), code)
        want = 1 if (env["FX_EISENSTAT"] == 1 and env.get("FX_SSOR_MODE", 1) == 1) else 0
        assert ctx.stats()["eisenstat"] == want, tag_of(env)
        try:
            check_solve(ctx.info, ctx.history, m.X, o["iter"], o["history"], o["X"], 1, printed=False)
        except AssertionError as e:
            raise AssertionError(tag_of(env)) from e
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------
# level-scheduled sweeps: ILU(0) (pc = 10) and the natural-order SSOR (FX_SSOR_NATURAL=1)
# ------------------------------------------------------------------------------------------------------------------------
LEVEL_VARIANTS = [
    (dict(FX_DATAFLOW=0), "split8"),                                         # launch per level, wave-split (8 waves)
    (dict(FX_DATAFLOW=0, FX_SPLIT_WPS=2), None),
    (dict(FX_DATAFLOW=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=64), "color"),    # launch per level, k_ssor_color
    (dict(FX_DATAFLOW=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=256, FX_SSOR_SPW=3), "color"),
    (dict(FX_DATAFLOW=0, FX_SPLIT_MAX_SLICES=0, FX_SSOR_BS=64, FX_SSOR_SPW=8, FX_PIPE_SSOR=0), None),
    (dict(FX_DATAFLOW=1), "split8"),                                         # one dataflow launch per apply
    (dict(FX_DATAFLOW=1, FX_DF_SOA=0, FX_DF_SLEEP=2, FX_DF_PRESLEEP=5, FX_DF_POLL=1), "split8"),
    (dict(FX_DATAFLOW=1, FX_DF_SOA=1, FX_DF_SLEEP=2, FX_DF_PRESLEEP=0, FX_DF_POLL=0), "split8"),
    (dict(FX_DATAFLOW=1, FX_DF_SOA=0, FX_DF_SLEEP=0, FX_DF_PRESLEEP=0, FX_DF_POLL=1), "split8"),
    (dict(FX_DATAFLOW=1, FX_DF_SOA=1, FX_DF_SLEEP=0, FX_DF_PRESLEEP=5, FX_DF_POLL=1), "split8"),
]


@pytest.mark.parametrize("shape", ["cube_c10", "hub"])
@pytest.mark.parametrize("kind", ["ilu0", "natural_ssor"])
def test_level_sweep_variants(hip, oracle, shapes, shape, kind, monkeypatch):
    """Apply against the oracle's (bit-groups as in the module docstring) and, on the cube, a BiCGSTAB solve against the oracle's
    (natural-order SSOR: the reference's one-thread branch, so the oracle runs with nthreads = 1)."""
    S = shapes[shape]
    pc, nthr = (10, 4) if kind == "ilu0" else (1, 1)
    zo = S.once("apply_" + kind, lambda: oracle.Precond(S.A, pc, ncolor_in=S.ncolor_in, nthreads=nthr).apply(S.r))
    I, R = S.params(2, pc)
    solve = shape != "hub"
    o = S.once("bicgstab_" + kind, lambda: oracle.solve_iterative(S.A, I, R, nthreads=nthr)) if solve else None
    groups = {}
    for env, grp in LEVEL_VARIANTS:
        if kind == "natural_ssor":
            env = dict(env, FX_SSOR_NATURAL=1)
        ctx = fresh_ctx(hip, monkeypatch, env)
        m = to_hecmat(hip, S.A)
        m.Iarray[:] = I; m.Rarray[:] = R
        ctx.upload(m)
        ctx.precond_setup(m)
        z = ctx.precond_apply(S.r)
        st = ctx.stats()
        assert st["df_mode"] == env["FX_DATAFLOW"] and st["df_fallbacks"] == 0 and st["ssor_natural"] == (kind != "ilu0")
        assert relerr(z[:3 * S.A.N], zo[:3 * S.A.N]) < 1e-12, tag_of(env)
        if grp is not None:
            ref = groups.setdefault(grp, z[:3 * S.A.N])
            assert np.array_equal(z[:3 * S.A.N], ref), (grp, tag_of(env))
        if solve:
            code = hip.hecmw_solve(None, m, ctx=ctx)
            assert code == 0 and m.Iarray[80] == 1, (tag_of(env), code)
            try:
                check_solve(ctx.info, ctx.history, m.X, o["iter"], o["history"], o["X"], 2, printed=False)
            except AssertionError as e:
                raise AssertionError(tag_of(env)) from e
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------------
# a switch flipped on a live context gives what a fresh context created with it gives
# ------------------------------------------------------------------------------------------------------------------------
# (option, value, method, precond, set-up time): "set-up time" options are followed by fx_precond_setup on the live context
LIVE_OPTIONS = [
    ("FX_PIPE_SPMV", 0, 1, 3, False),
    ("FX_SPMV_BS", 64, 1, 3, False),
    ("FX_SPMV_SPATIAL", 0, 1, 1, False),
    ("FX_SSOR_MODE", 0, 1, 1, True),
    ("FX_SPLIT_MAX_SLICES", 0, 1, 1, False),
    ("FX_SSOR_BS", 256, 1, 1, False),
    ("FX_PIPE_SSOR", 0, 1, 1, False),
    ("FX_SSOR_SPW", 3, 1, 1, False),
    ("FX_PIPE_MAX_SLICES", 12, 1, 1, False),
    ("FX_SPLIT_WPS", 8, 1, 1, False),
    ("FX_EISENSTAT", 0, 1, 1, False),
    ("FX_EIS_FUSE", 0, 1, 1, False),
    ("FX_EIS_MERGE", 0, 1, 1, False),
    ("FX_EIS_GRID", 3, 1, 1, False),
    ("FX_DATAFLOW", 0, 2, 10, False),
    ("FX_DATAFLOW", 2, 1, 1, False),
    ("FX_DF_SOA", 0, 2, 10, False),
    ("FX_DF_POLL", 1, 2, 10, False),
    ("FX_DF_SLEEP", 2, 2, 10, False),
    ("FX_DF_PRESLEEP", 5, 2, 10, False),
    ("FX_DF_WPS", 4, 2, 10, False),
    ("FX_SSOR_NATURAL", 1, 2, 1, False),
    ("FX_LAYOUT_DEVICE", 0, 1, 1, True),
]
# options whose live flip needs a non-default base to mean anything: FX_DATAFLOW=2 under the natural-order Krylov vectors, the
# slice walk of the SpMV in the standard loop (whose p.q partials it groups), k_ssor_color's knobs with the non-split sweeps
LIVE_BASE = {("FX_DATAFLOW", 2): dict(FX_SSOR_MODE=0), ("FX_SPMV_SPATIAL", 0): dict(FX_EISENSTAT=0), ("FX_PIPE_MAX_SLICES", 12): dict(FX_SPLIT_MAX_SLICES=0),
             ("FX_SSOR_BS", 256): dict(FX_SPLIT_MAX_SLICES=0), ("FX_PIPE_SSOR", 0): dict(FX_SPLIT_MAX_SLICES=0),
             ("FX_SSOR_SPW", 3): dict(FX_SPLIT_MAX_SLICES=0)}


def test_live_switches_give_the_answer_a_fresh_context_gives(hip, oracle, shapes, monkeypatch):
    """For every option of the variant table: solve with the base settings, flip the option on the SAME context (fx_set_option),
    run fx_precond_setup if it is a set-up-time option, solve again from X = 0 with the preconditioner kept (Iarray(97) = Iarray(98) = 0):
    X, history and count must equal, bit for bit, those of a fresh context created with the option in its environment.
    FX_SSOR_MODE is the set-up-time one (the numbering of the multicolour SSOR, include/fistr_hip.h); FX_DATAFLOW=2 under
    FX_SSOR_MODE=0 needs the private backward vector the set-up did not allocate; FX_SPMV_SPATIAL / FX_SPMV_BS re-walk a resident
    layout; FX_LAYOUT_DEVICE only matters for the next build."""
    S = shapes["cube_c10"]

    def system(meth, pc):
        I, R = S.params(meth, pc, SIGMA if pc == 1 else 1.0)
        m = to_hecmat(hip, S.A)
        m.Iarray[:] = I; m.Rarray[:] = R
        return m

    def solve(ctx, m):
        m.X[:] = 0.0
        code = hip.hecmw_solve(None, m, ctx=ctx)
        assert code == 0 and m.Iarray[80] == 1
        m.Iarray[96] = 0; m.Iarray[97] = 0              # the second solve keeps the matrix and the preconditioner
        return m.X.copy(), ctx.history.copy(), ctx.info.iterations, ctx.stats()["eisenstat"]

    assert {o[0] for o in LIVE_OPTIONS} <= set(VARIANT_ENV)
    for name, value, meth, pc, setup in LIVE_OPTIONS:
        base = LIVE_BASE.get((name, value), {})
        fresh = fresh_ctx(hip, monkeypatch, dict(base, **{name: value}))
        want = solve(fresh, system(meth, pc))
        fresh.close()
        ctx = fresh_ctx(hip, monkeypatch, base)
        m = system(meth, pc)
        solve(ctx, m)
        ctx.set_option(name, value)
        if setup:
            ctx.precond_setup(m)
        got = solve(ctx, m)
        ctx.close()
        assert got[2] == want[2] and got[3] == want[3], (name, value, got[2:], want[2:])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, value)


def test_live_ssor_mode_change_needs_the_set_up(hip, shapes, monkeypatch):
    """FX_SSOR_MODE changed on a context with a resident multicolour SSOR: the preconditioner is reported as not set up (instead
    of applying the one built in the other numbering) until fx_precond_setup rebuilds it -- then it equals a fresh context's."""
    S = shapes["cube_c10"]
    m = to_hecmat(hip, S.A)
    m.Iarray[2] = 1; m.Iarray[33] = S.ncolor_in; m.Rarray[1] = SIGMA
    fresh = fresh_ctx(hip, monkeypatch, dict(FX_SSOR_MODE=0))
    fresh.upload(m)
    fresh.precond_setup(m)
    want = fresh.precond_apply(S.r)
    fresh.close()
    ctx = fresh_ctx(hip, monkeypatch, {})
    ctx.upload(m)
    ctx.precond_setup(m)
    ctx.precond_apply(S.r)
    ctx.set_option("FX_SSOR_MODE", 0)
    with pytest.raises(hip.HecmwSolverError):
        ctx.precond_apply(S.r)
    ctx.precond_setup(m)
    assert np.array_equal(ctx.precond_apply(S.r), want)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------
# the value arena's verification walk, at the size where it runs
# ------------------------------------------------------------------------------------------------------------------------
def test_arena_walk_keeps_the_answers_bit_identical(hip, monkeypatch):
    """81^3 = 531,441 rows (1.6 M DOF, >= 8,192 slices in M: the size from which arena_verify times the SpMV on the arena), device
    assembly; needs about 6 GiB of device memory.  FX_ARENA_THRESHOLD_MB=0 + a small FX_ARENA_GB put M / L / U in an arena,
    FX_ARENA_TRIES=3 + FX_ARENA_GOOD_GBS=1e9 make the verification walk every arena (each one re-points the value arrays and
    refills M) and switch back to the fastest.  CG + SSOR in both forms and BiCGSTAB + ILU(0), then new values (FX_UP_VALUES,
    preconditioner rebuilt) and a recycled preconditioner: every X / history bit-identical to the same sequence without an arena."""
    from frontistr_amd.mesh import CubeMesh
    mesh = CubeMesh(80)
    load = mesh.load()

    def run(arena_gb):
        ctx = fresh_ctx(hip, monkeypatch, {})
        for k, v in (("FX_ARENA_THRESHOLD_MB", 0), ("FX_ARENA_GB", arena_gb), ("FX_ARENA_TRIES", 3), ("FX_ARENA_GOOD_GBS", 1e9)):
            ctx.set_option(k, v)
        hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
        hm.elem_node_item = mesh.conn.ravel()
        m = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ctx.upload(m, what=hip.FX_UP_PROFILE)
        ctx.assemble_c3d8(mesh.coord, mesh.conn, 210000.0, 0.3, elemopt=1, load=load, bc=mesh.dirichlet())
        ctx.download_matrix(m)
        out = []

        def solve(meth, pc, eis, flags):
            ctx.set_option("FX_EISENSTAT", eis)
            m.Iarray[0] = 10000; m.Iarray[1] = meth; m.Iarray[2] = pc; m.Iarray[4] = 1
            m.Iarray[96], m.Iarray[97] = flags
            m.X[:] = 0.0
            ctx.upload(m, what=hip.FX_UP_X)
            code = ctx.solve_resident(m)
            ctx.download_x(m)
            assert code == 0 and m.Iarray[80] == 1, (meth, pc, eis, code)
            out.append((m.X.copy(), ctx.history.copy(), ctx.info.iterations, ctx.stats()["eisenstat"]))

        solve(1, 1, 1, (1, 1))
        p = ctx.placement_report()
        solve(1, 1, 0, (0, 0))
        solve(2, 10, 1, (1, 1))
        D0 = m.D.copy()
        m.D[:] = D0 * 1.05                                           # new values: the preconditioner is rebuilt from them
        ctx.upload(m, what=hip.FX_UP_VALUES)
        solve(1, 1, 1, (1, 1))
        m.D[:] = D0 * 1.1                                            # new values, recycled preconditioner (standard loop)
        ctx.upload(m, what=hip.FX_UP_VALUES)
        solve(1, 1, 1, (0, 0))
        p2 = ctx.placement_report()
        ctx.close()
        return out, p, p2

    got, p, p2 = run(1.0 / 64)
    assert p["arenas_timed"] == 3 and p2["arenas_timed"] == 3, (p, p2)
    assert p["spmv_values_in_arena"] and p["lower_values_in_arena"] and p["upper_values_in_arena"]
    want, q, _ = run(0)
    assert q["arena_bytes"] == 0 and q["arenas_timed"] == 0
    assert [g[3] for g in got] == [1, 0, 0, 1, 0]                    # the forms asked for (a recycled preconditioner: standard loop)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2] and g[3] == w[3], k
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]), k
