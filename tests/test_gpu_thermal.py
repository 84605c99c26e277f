"""Thermal strain of a linear static analysis on the device: fx_thermal_load_groups (TLOAD_C3 / TLOAD_C3D8Bbar / TLOAD_C3D8IC) and
fx_update_groups_linear_thermal (the thermal branches of UPDATE_C3 / Update_C3D8Bbar / UpdateST_C3D8IC) against the numpy
restatement tests/thermal_ref.py, per type and elemopt.

Tolerances are those of the linear update tests of each type: 1e-12 of the largest entry for strain and stress and 1e-11 for the
vectors summed with fp64 atomics at 341 / 342 / 351 / 352 / 362 (test_gpu_tet_assembly.py, test_gpu_c3_assembly.py), 1e-11 throughout
at 361 (test_oracle_update.py, fx_update_linear.h) and on the mixed mesh (test_gpu_mixed_assembly.py).  The load vector is added
with fp64 atomics, like QFORCE, so two calls agree to that rounding, not bit for bit; what is bit for bit is strain and stress
from call to call, one group alone against its part of a mixed call (the single-type kernels against the groups path), and the
update with a temperature that causes no thermal strain against the update without one.

Every test here fails without the feature: the library has no fx_thermal_load_groups / fx_update_groups_linear_thermal.
Meshes: (a) one distorted element with all node temperatures different, (b) an element count that is no multiple of the elements
per workgroup of the type's update kernel (361: 32; 341: 256, 342: 64; 351: 32, 352: 8, 362: 2), (c) two materials with
different expansion coefficients, (d) MixedMesh(2) of both orders through the groups entry points."""
import ctypes as C

import numpy as np
import pytest

import thermal_ref as TH
from frontistr_amd import hecmw as hip
from frontistr_amd.mesh import CubeMesh, MixedMesh, mesh_groups, solid_mesh

pytestmark = pytest.mark.gpu
E2, NU2, AL2 = np.array([210000.0, 70000.0]), np.array([0.3, 0.33]), np.array([1.2e-5, 2.3e-5])
REF_T = 20.0
# (etype, elemopt) -> (strain / stress bound, vector bound)
CASES = [(361, 1), (361, 2), (361, 3), (341, 1), (342, 1), (351, 1), (352, 1), (362, 1)]


def _tol(etype):
    return (1e-11, 1e-11) if etype == 361 else (1e-12, 1e-11)


def _mesh(etype, n):
    if etype == 361:
        m = CubeMesh(n, skew=0.1)
        m.etype = 361
        return m
    return solid_mesh(n, etype, skew=0.1, **({} if etype in (341, 351) else {"curve": 0.03}))


def _fields(m, seed):
    rng = np.random.default_rng(seed)
    temp = 20.0 + 150.0 * rng.random(m.n_node)          # every node another temperature
    temp0 = 20.0 + 10.0 * rng.random(m.n_node)
    disp = 2.0e-3 * (rng.random(3 * m.n_node) - 0.5)
    return temp, temp0, disp


# per type the smallest cube that fills more than one workgroup of the update kernel and whose element count is no multiple of
# its elements per workgroup: 361 5^3 = 125 = 3 x 32 + 29; 341 6 x 4^3 = 384 = 256 + 128; 342 6 x 3^3 = 162 = 2 x 64 + 34;
# 351 / 352 2 x 3^3 = 54 = 32 + 22 = 6 x 8 + 6; 362 3^3 = 27 = 13 x 2 + 1
SIZES = {361: (1, 5), 341: (1, 4), 342: (1, 3), 351: (1, 3), 352: (1, 3), 362: (1, 3)}
EPB = {361: 32, 341: 256, 342: 64, 351: 32, 352: 8, 362: 2}


@pytest.fixture(scope="module")
def ctx():
    c = hip.SolverContext(device=0)
    yield c
    c.close()


def _check(ctx, etype, elemopt, m, E, nu, alpha, em, seed):
    temp, temp0, disp = _fields(m, seed)
    th = (temp, temp0, REF_T, alpha)
    groups = mesh_groups(m, elemopt, em)
    te, tv = _tol(etype)
    f, _ = ctx.thermal_load_groups(m.coord, groups, E, nu, th)
    rf = TH.thermal_load(m.coord, groups, E, nu, th)
    print("etype %d elemopt %d n_elem %d: load err %.2e" % (etype, elemopt, m.n_elem, np.abs(f - rf).max() / np.abs(rf).max()))
    assert np.abs(f - rf).max() <= tv * np.abs(rf).max()
    s, st, q, _ = ctx.update_groups_linear(m.coord, groups, E, nu, disp, thermal=th)
    rs, rst, rq = TH.update(m.coord, groups, E, nu, disp, th)
    print("   strain %.2e stress %.2e qforce %.2e" % (np.abs(s[0] - rs[0]).max() / np.abs(rs[0]).max(),
                                                     np.abs(st[0] - rst[0]).max() / np.abs(rst[0]).max(), np.abs(q - rq).max() / np.abs(rq).max()))
    assert np.abs(s[0] - rs[0]).max() <= te * np.abs(rs[0]).max()
    assert np.abs(st[0] - rst[0]).max() <= te * np.abs(rst[0]).max()
    assert np.abs(q - rq).max() <= tv * np.abs(rq).max()
    return th, groups, disp, f, s, st


@pytest.mark.parametrize("etype,elemopt", CASES)
def test_one_distorted_element(ctx, etype, elemopt):
    m = _mesh(etype, 1)
    if etype not in (361, 362):        # the cube of one cell holds several tetrahedra / wedges: keep the first
        m.conn = np.ascontiguousarray(m.conn[:1]); m.n_elem = 1
    rng = np.random.default_rng(3)
    m.coord = m.coord + 0.08 * (rng.random(m.coord.shape) - 0.5)
    _check(ctx, etype, elemopt, m, 210000.0, 0.3, 1.2e-5, None, 5)


@pytest.mark.parametrize("etype,elemopt", CASES)
def test_idle_lanes_and_two_materials(ctx, etype, elemopt):
    """(b) and (c): an element count that leaves lanes of the last workgroup idle, two materials with different alpha."""
    m = _mesh(etype, SIZES[etype][1])
    assert m.n_elem % EPB[etype] != 0 and m.n_elem > EPB[etype]
    em = np.where(np.arange(m.n_elem) % 3 == 0, 2, 1).astype(np.int32)
    th, groups, disp, f, s, st = _check(ctx, etype, elemopt, m, E2, NU2, AL2, em, 7)
    # a second call, through the single-mesh convenience (the same group, the same kernels): strain and stress are each one
    # lane's own sums, so they repeat bit for bit; only the vectors added with atomics may differ in rounding
    s1, st1, _, _ = ctx.update_linear(m, E2, NU2, disp, elemopt=elemopt, elem_mat=em, thermal=th)
    assert np.array_equal(s1[0], s[0]) and np.array_equal(st1[0], st[0])
    # added to the caller's vector, which itself stays as it was
    base = np.linspace(-1.0, 1.0, 3 * m.n_node)
    keep = base.copy()
    f2, _ = ctx.thermal_load(m, E2, NU2, th, elemopt=elemopt, elem_mat=em, load=base)
    assert np.array_equal(base, keep)
    assert np.abs(f2 - (base + f)).max() <= 1e-11 * np.abs(f).max()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("elemopt", [1, 2, 3])
def test_mixed_mesh_through_the_groups(ctx, order, elemopt):
    m = MixedMesh(2, order=order, skew=0.1, curve=0.03 if order == 2 else 0.0)
    em = np.where(np.arange(m.n_elem) % 2 == 0, 1, 2).astype(np.int32)
    groups = m.groups_with(elemopt, em)
    temp, temp0, disp = _fields(m, 11)
    th = (temp, temp0, REF_T, AL2)
    f, _ = ctx.thermal_load_groups(m.coord, groups, E2, NU2, th)
    rf = TH.thermal_load(m.coord, groups, E2, NU2, th)
    assert np.abs(f - rf).max() <= 1e-11 * np.abs(rf).max()
    s, st, q, _ = ctx.update_groups_linear(m.coord, groups, E2, NU2, disp, thermal=th)
    rs, rst, rq = TH.update(m.coord, groups, E2, NU2, disp, th)
    for g in range(len(groups)):
        assert np.abs(s[g] - rs[g]).max() <= 1e-11 * np.abs(rs[g]).max(), g
        assert np.abs(st[g] - rst[g]).max() <= 1e-11 * np.abs(rst[g]).max(), g
    assert np.abs(q - rq).max() <= 1e-11 * np.abs(rq).max()
    # every group alone (the single-type kernels) gives the same numbers as its part of the mixed call, bit for bit
    for g, grp in enumerate(groups):
        s1, st1, _, _ = ctx.update_groups_linear(m.coord, [grp], E2, NU2, disp, thermal=th)
        assert np.array_equal(s1[0], s[g]) and np.array_equal(st1[0], st[g]), g


@pytest.mark.parametrize("etype,elemopt", CASES)
def test_no_thermal_strain_is_the_plain_update(ctx, etype, elemopt):
    """temp == temp0 == ref_temp: a zero load vector, and strain and stress bit for bit those of fx_update_groups_linear.

    The IC element's stored stress is written with its fused multiply-adds spelled out (iso_stress_fixed) in both instantiations of
    its kernel: left to the compiler, the two contracted D (strain - 0) and D strain differently and differed in the last place."""
    m = _mesh(etype, 2)
    _, _, disp = _fields(m, 13)
    t = np.full(m.n_node, REF_T)
    th = (t, t, REF_T, 1.2e-5)
    groups = mesh_groups(m, elemopt)
    f, _ = ctx.thermal_load_groups(m.coord, groups, 210000.0, 0.3, th)
    assert not f.any()
    s, st, q, _ = ctx.update_groups_linear(m.coord, groups, 210000.0, 0.3, disp, thermal=th)
    s0, st0, q0, _ = ctx.update_groups_linear(m.coord, groups, 210000.0, 0.3, disp)
    print("etype %d elemopt %d: strain differs by %.2e, stress by %.2e of the largest entry"
          % (etype, elemopt, np.abs(s[0] - s0[0]).max() / np.abs(s0[0]).max(), np.abs(st[0] - st0[0]).max() / np.abs(st0[0]).max()))
    assert np.array_equal(s[0], s0[0]) and np.array_equal(st[0], st0[0])
    assert np.abs(q - q0).max() <= 1e-11 * np.abs(q0).max()          # (fp64 atomics: the order of the additions is free)


@pytest.mark.parametrize("etype,elemopt", CASES)
def test_equilibrium(ctx, etype, elemopt):
    """Assemble, add the thermal load, solve (CG + SSOR, RESID 1e-8), update: QFORCE balances the applied load at every free dof
    to the solver's RESID, relative to the norm of the right-hand side (mechanical + thermal load) the solver measures its
    residual against."""
    m = _mesh(etype, 3 if etype in (361, 341, 351) else 2)
    temp, temp0, _ = _fields(m, 17)
    if (etype, elemopt) == (361, 2):
        # TLOAD_C3D8Bbar takes the thermal strain of every point from the centroid's temperatures (C3D8.f90:607-608, :688) and
        # Update_C3D8Bbar from the point's own (:311-343): the reference's load and internal force balance only where the two
        # agree, so the B-bar case runs with one temperature for all nodes (the restatement shows the same imbalance otherwise)
        temp, temp0 = np.full(m.n_node, 135.0), np.full(m.n_node, 25.0)
    th = (temp, temp0, REF_T, 1.2e-5)
    groups = mesh_groups(m, elemopt)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    mat = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    c = hip.SolverContext(device=0)
    try:
        c.upload(mat, what=hip.FX_UP_PROFILE)
        rhs, _ = c.thermal_load_groups(m.coord, groups, 210000.0, 0.3, th, load=m.load())
        bc = m.dirichlet()
        c.assemble_groups(m.coord, groups, 210000.0, 0.3, load=rhs, bc=bc)
        mat.Iarray[0], mat.Iarray[1], mat.Iarray[2] = 10000, 1, 1
        mat.Rarray[0] = 1.0e-8
        assert c.solve_resident(mat) == 0
        c.download_x(mat)
        _, _, q, _ = c.update_groups_linear(m.coord, groups, 210000.0, 0.3, mat.X, thermal=th)
    finally:
        c.close()
    free = np.ones(3 * m.n_node, dtype=bool)
    free[3 * (bc[0] - 1) + bc[1] - 1] = False
    res = np.linalg.norm((q - m.load())[free]) / np.linalg.norm(rhs[free])
    print("etype %d elemopt %d: |qforce - load| / |rhs| = %.2e" % (etype, elemopt, res))
    # the free rows of the eliminated system are K u = rhs (the prescribed values are zero, its fixed rows hold 0 = 0), so the
    # balance is the solver's relative residual |r| / |b|, which the linear fistr1 tests hold to the deck's RESID
    # (test_gpu_fistr1.py: `### Relative residual` <= 1e-8)
    assert res <= 1.0e-8


@pytest.mark.parametrize("etype,elemopt", CASES)
def test_equal_temperatures_away_from_ref_temp_give_no_load(ctx, etype, elemopt):
    """temp == temp0 at every node, neither equal to ref_temp: alp (TEMPC - ref) - alp (TEMP0 - ref) is the difference of two
    equal rounded products, so the load vector is exactly zero -- unless a product is fused into the subtraction."""
    m = _mesh(etype, 2)
    temp, _, _ = _fields(m, 23)
    f, _ = ctx.thermal_load_groups(m.coord, mesh_groups(m, elemopt), 210000.0, 0.3, (temp, temp.copy(), REF_T, 1.2e-5))
    assert not f.any()


def test_refusals_write_nothing(ctx):
    m = _mesh(341, 1)
    temp, temp0, disp = _fields(m, 19)
    groups = mesh_groups(m)
    load = np.arange(3.0 * m.n_node)
    for th, what in (((None, temp0, REF_T, 1e-5), "temperature"), ((temp, None, REF_T, 1e-5), "temperature"),
                     ((temp, temp0, REF_T, None), "expansion")):
        keep = load.copy()
        with pytest.raises(hip.HecmwSolverError, match=what) as e:
            ctx.thermal_load_groups(m.coord, groups, 210000.0, 0.3, th, load=load)
        assert e.value.code == -1 and np.array_equal(load, keep)
        with pytest.raises(hip.HecmwSolverError, match=what):
            ctx.update_groups_linear(m.coord, groups, 210000.0, 0.3, disp, thermal=th)
        # the update writes nothing either: the C entry point itself, with the caller's qforce and result pointers filled beforehand
        tab, keep = ctx._group_table(groups)
        tv, keep_t = ctx._thermal_view(th)
        Es, nus = np.array([210000.0]), np.array([0.3])
        qf = np.arange(3.0 * m.n_node)
        ps, pt = (C.c_void_p * 1)(12345), (C.c_void_p * 1)(12345)
        rc = hip.lib().fx_update_groups_linear_thermal(ctx.h, m.n_node, hip._ptr(m.coord), 1, tab, 1, hip._ptr(Es), hip._ptr(nus),
                                                       C.byref(tv), hip._ptr(disp), ps, pt, hip._ptr(qf), None)
        assert rc == -1 and np.array_equal(qf, np.arange(3.0 * m.n_node)) and ps[0] == 12345 and pt[0] == 12345
    th = (temp, temp0, REF_T, 1e-5)
    for call in (lambda g: ctx.thermal_load_groups(m.coord, g, 210000.0, 0.3, th),
                 lambda g: ctx.update_groups_linear(m.coord, g, 210000.0, 0.3, disp, thermal=th)):
        with pytest.raises(hip.HecmwSolverError) as e:
            call([(371, m.conn, 1, None)])
        assert e.value.code == -2
