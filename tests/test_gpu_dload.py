"""Distributed loads on the device (csrc/fx_dload.h: fx_dload_element, fx_dload_groups) against the numpy restatement of DL_C3
(tests/dload_ref.py) and against the known answers of the reference's example decks exB..exE for the six solid types.

Bounds: one element without atomics 1e-12 of the largest entry, atomically summed vectors 1e-11 of the largest entry (the
project's bounds for element quantities and for scattered sums).

Meshes: the 5^3 cube.  The face kernels take 8 faces per workgroup and a cube side has 25 quadrilaterals or 50 triangles; the
volume kernels take 64 / 16 / 32 / 16 / 32 / 8 elements per workgroup (341 / 342 / 351 / 352 / 361 / 362) and the cube has 750
tetrahedra, 250 wedges or 125 hexahedra: every kernel runs more than one workgroup and a partial last one.  WedgeMesh has its
triangles on the z sides and its quadrilaterals on the others, so no single side mixes the two: its list takes the top side
and the x = 5 side.  MixedMesh's top side holds quadrilaterals (the x-axis wedges) and triangles (the tetrahedra)."""
import ctypes as C

import numpy as np
import pytest

import dload_ref as R
from dload_decks import DECKS, dload_arrays, read_deck
from frontistr_amd.mesh import CubeMesh, MixedMesh, mesh_groups, solid_mesh
from test_dload_ref import TYPES, skewed_element

pytestmark = pytest.mark.gpu
FX_ERROR_UNSUPPORTED, FX_ERROR_RUNTIME = -2, -1
RHO = np.array([7.8, 2.7])
# the decks on which CG + DIAG cannot confirm 1e-10 (test_example_decks_known_answers says why); every other deck must converge
UNCONFIRMED = {(ex, t) for ex in "BCD" for t in (342, 352)}


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.SolverContext()
    yield c
    c.close()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("etype", TYPES)
def test_element(ctx, etype):
    """Every (type, LTYPE): 1..5 and every face, one skewed element with curved mid-edge nodes."""
    X, _ = skewed_element(etype, curve=0.07)
    cases = [(1, [3.0]), (2, [-2.0]), (3, [1.5]), (4, [9.8, 1.0, -2.0, 2.0]), (5, [3.0, 0.5, -1.0, 0.25, 1.0, 2.0, -0.5])]
    cases += [(10 * f, [2.5]) for f in range(1, len(R.SUBFACE[etype]) + 1)]
    for ltype, p in cases:
        par = np.array(list(p) + [0.0] * (7 - len(p)))
        want = R.dl_c3(etype, X, 7.8, ltype, par)
        got = ctx.dload_element(etype, ltype, X, par, rho=7.8)
        err = _rel(got, want)
        print("TYPE=%d LTYPE=%d: %.3e" % (etype, ltype, err))
        assert err <= 1e-12, (etype, ltype, err)
        if ltype >= 10:     # VECT is zero off the face
            off = np.setdiff1d(np.arange(R.NODES[etype]), np.array(R.SUBFACE[etype][ltype // 10 - 1]) - 1)
            assert not got.reshape(-1, 3)[off].any()


def _mesh(name):
    if name == "mixed":
        m = MixedMesh(5, skew=0.15)
    elif name == 361:
        m = CubeMesh(5, skew=0.15)
    else:
        m = solid_mesh(5, name, skew=0.15, **({"curve": 0.05} if name in (342, 352, 362) else {}))
    n_elem = sum(np.asarray(g[1]).shape[0] for g in mesh_groups(m))
    em = (1 + (np.arange(n_elem) * 7 // 3) % 2).astype(np.int32)
    return m, mesh_groups(m, 1, em)


def _list(m, groups, name):
    """pressure on a cube side, GRAV on all elements, CENT on a subset, one BX entry twice, one held entry"""
    on = m.coord[:, 2] == 5.0
    sides = [on] + ([m.coord[:, 0] == 5.0] if name in (351, 352) else [])
    cards = []
    for mask in sides:
        for g, e, f in R.boundary_faces([gr[:2] for gr in groups]):
            nod = np.asarray(groups[g][1])[e, np.array(R.SUBFACE[groups[g][0]][f - 1]) - 1] - 1
            if mask[nod].all():
                cards.append((g, [e], 10 * f, [1.5]))
    for g, gr in enumerate(groups):
        ne = np.asarray(gr[1]).shape[0]
        cards.append((g, np.arange(ne), 4, [9.8, 0.3, -0.2, -1.0]))
        cards.append((g, np.arange(0, ne, 3), 5, [2.0, 2.5, 2.5, 0.0, 0.1, -0.2, 1.0]))
    cards += [(0, [1], 1, [4.0]), (0, [1], 1, [4.0]), (0, [2], 2, [6.0], True)]
    return R.entries(*cards)


@pytest.mark.parametrize("name", list(TYPES) + ["mixed"])
def test_mesh(ctx, name):
    m, groups = _mesh(name)
    dl = _list(m, groups, name)
    shapes = {R.NODES[groups[g][0]] if lt < 10 else len(R.SUBFACE[groups[g][0]][lt // 10 - 1]) for g, lt in zip(dl[0], dl[2])}
    if name in (351, 352, "mixed"):
        assert {3, 4} <= shapes or {6, 8} <= shapes         # the list mixes triangles and quadrilaterals
    want = R.assemble(m.coord, groups, RHO, dl, factor=0.5)
    got, ms = ctx.dload_groups(m.coord, groups, RHO, dl, factor=0.5)
    print("%s: %d entries, %.3e of the largest entry, %.3f ms" % (name, len(dl[0]), _rel(got, want), ms))
    assert _rel(got, want) <= 1e-11
    st = ctx.dload_stats()
    assert st["tri_entries"] + st["quad_entries"] == int((dl[2] >= 10).sum())
    assert (st["body_entries"], st["grav_entries"], st["cent_entries"]) == tuple(int((dl[2] == k).sum()) if k > 3 else
                                                                                 int((dl[2] <= 3).sum()) for k in (3, 4, 5))
    assert st["lanes_per_face"] == 8
    # added to, not overwritten
    base = np.sin(np.arange(want.size) * 0.37) * np.abs(want).max()
    got2, _ = ctx.dload_groups(m.coord, groups, RHO, dl, factor=0.5, load=base)
    assert np.abs(got2 - (base + want)).max() <= 1e-11 * np.abs(want).max()
    # on the displaced configuration
    disp = 0.02 * np.cos(np.arange(want.size) * 0.61)
    want_d = R.assemble(m.coord, groups, RHO, dl, factor=0.5, disp=disp)
    got_d, _ = ctx.dload_groups(m.coord, groups, RHO, dl, factor=0.5, disp=disp)
    assert _rel(got_d, want_d) <= 1e-11
    assert _rel(want_d, want) > 1e-3


def _raw(hip, ctx, coord, groups, rho, dl, load, null=None):
    """fx_dload_groups itself, on the caller's own vector; null: the member of fx_dload to pass as NULL"""
    tab, keep = hip.SolverContext._group_table(groups)
    dv, keep_d = hip.SolverContext._dload(dl)
    if null:
        setattr(dv, null, None)
    rho = None if rho is None else np.ascontiguousarray(rho, dtype=np.float64)
    coord = np.ascontiguousarray(coord, dtype=np.float64)
    code = hip.lib().fx_dload_groups(ctx.h, int(coord.shape[0]), hip._ptr(coord), len(groups), tab, 0 if rho is None else rho.size,
                                     hip._ptr(rho), C.byref(dv), C.c_double(0.5), None, hip._ptr(load), None)
    del keep, keep_d
    return code, hip.lib().fx_last_error().decode()


def test_refusals_leave_the_vector_alone(hip, ctx):
    m = MixedMesh(2)
    groups = mesh_groups(m)                     # 361, 351, 341
    load = np.sin(np.arange(3 * m.n_node) * 0.3)
    keep = load.copy()
    ok = R.entries((0, [0], 20, [1.0]), (1, [0], 4, [9.8, 0, 0, -1]))
    bad = [
        ("unknown type", [(343, groups[0][1])] + groups[1:], RHO[:1], ok, None, FX_ERROR_UNSUPPORTED, "343"),
        ("no such volume load", groups, RHO[:1], R.entries((0, [0], 6, [1.0])), None, FX_ERROR_RUNTIME, "entry 1"),
        ("no LTYPE 15", groups, RHO[:1], R.entries((0, [0], 20, [1.0]), (0, [0], 15, [1.0])), None, FX_ERROR_RUNTIME, "entry 2"),
        ("a hexahedron has no face 7", groups, RHO[:1], R.entries((0, [0], 70, [1.0])), None, FX_ERROR_RUNTIME, "TYPE=361"),
        ("a wedge has no face 6", groups, RHO[:1], R.entries((1, [0], 60, [1.0])), None, FX_ERROR_RUNTIME, "group 2"),
        ("a tetrahedron has no face 5", groups, RHO[:1], R.entries((2, [0], 50, [1.0])), None, FX_ERROR_RUNTIME, "group 3"),
        ("group out of range", groups, RHO[:1], R.entries((3, [0], 1, [1.0])), None, FX_ERROR_RUNTIME, "group out of range"),
        ("negative group", groups, RHO[:1], R.entries((-1, [0], 1, [1.0])), None, FX_ERROR_RUNTIME, "group out of range"),
        ("element out of range", groups, RHO[:1], R.entries((0, [np.asarray(groups[0][1]).shape[0]], 1, [1.0])), None, FX_ERROR_RUNTIME,
         "is not in group 1"),
        ("negative element", groups, RHO[:1], R.entries((0, [-1], 1, [1.0])), None, FX_ERROR_RUNTIME, "is not in group 1"),
        ("null params", groups, RHO[:1], ok, "params", FX_ERROR_RUNTIME, "arrays missing"),
        ("null ltype", groups, RHO[:1], ok, "ltype", FX_ERROR_RUNTIME, "arrays missing"),
        ("GRAV without rho", groups, None, ok, None, FX_ERROR_RUNTIME, "need rho"),
        ("CENT without rho", groups, None, R.entries((0, [0], 5, [1.0, 0, 0, 0, 0, 0, 1])), None, FX_ERROR_RUNTIME, "need rho"),
        ("zero GRAV direction", groups, RHO[:1], R.entries((0, [0], 4, [9.8, 0, 0, 0])), None, FX_ERROR_RUNTIME, "zero direction"),
        ("zero CENT axis", groups, RHO[:1], R.entries((0, [0], 5, [1.0, 1, 2, 3, 0, 0, 0])), None, FX_ERROR_RUNTIME, "zero axis"),
    ]
    for tag, grp, rho, dl, null, code, text in bad:
        got, msg = _raw(hip, ctx, m.coord, grp, rho, dl, load, null)
        assert got == code, (tag, got, msg)
        assert text in msg, (tag, msg)
        assert np.array_equal(load, keep), tag
    got, msg = _raw(hip, ctx, m.coord, groups, RHO[:1], ok, load)
    assert got == 0, msg
    assert not np.array_equal(load, keep)
    with pytest.raises(hip.HecmwSolverError):
        ctx.dload_element(361, 70, np.zeros((8, 3)), np.zeros(7))
    with pytest.raises(hip.HecmwSolverError):
        ctx.dload_element(343, 1, np.zeros((8, 3)), np.zeros(7))


@pytest.mark.parametrize("ex,etype", DECKS)
def test_example_decks_known_answers(hip, ex, etype):
    """exB (pressure), exC (BZ), exD (GRAV), exE (CENT) for the six solid types: the device's distributed load, the device's
    assembly with the FIX boundary and CG give the displacement extrema of the shipped X3nn_correct.log -- which holds the face
    numbering of every type, 342 and 352 included, against the reference's own run."""
    from test_oracle_golden import check_extrema
    d = read_deck(ex, etype)
    coord, groups = d["coord"], d["groups"]
    hm = hip.hecmwST_local_mesh(n_node=coord.shape[0])
    m = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    c = hip.SolverContext()
    c.upload(m, what=hip.FX_UP_PROFILE)
    load, _ = c.dload_groups(coord, groups, d["rho"], dload_arrays(d["cards"]))
    assert np.abs(load).max() > 0.0
    bc = (np.repeat(d["fix"], 3).astype(np.int32), np.tile(np.array([1, 2, 3], dtype=np.int32), d["fix"].size), np.zeros(3 * d["fix"].size))
    c.assemble_groups(coord, groups, d["E"], d["nu"], load=load, bc=bc)
    # CG with the deck's preconditioner (DIAG in all of them), asked for 1e-10, within as many iterations as the system has
    # unknowns: the number at which CG ends in exact arithmetic.  The second-order beams have a condition number of 3.5e6 to 4.2e6
    # under DIAG, so b - A x cannot even be evaluated below eps * kappa = 4e-10 of |b| in fp64, and hecmw_solve_CG accepts an
    # iteration only when the true residual confirms it (hecmw_solver_CG.f90:259-266): on B342, C342, D342 and on B352, C352, D352
    # (by a hair, either way) it cannot confirm 1e-10 and runs to the cap, W-3001.  What it does beyond its floor is a walk: the
    # restatement of the reference's own loop (oracle/, on the host) leaves these systems at 3e-10 to 3e-9 after 3 NP iterations
    # and at 1.5e-9 (B342), 9e-8 (D342), 3e-7 (D352), 2.9e-4 (C352) and 2e-2 (B352, displacement extrema off) after the decks' own
    # 10000; the library gave 1.26e-8 on B342 there.  Hence the cap.  On these six decks the code may be 0 or 3001, on the other 18 it is 0; the true residual must be below
    # the 1e-8 the decks themselves ask for, and the displacements are judged as everywhere else.
    m.Iarray[0] = 3 * coord.shape[0]; m.Iarray[1] = 1; m.Iarray[2] = d["precond"] if d["precond"] in (1, 3, 10) else 3
    m.Rarray[0] = 1.0e-10
    code = c.solve_resident(m)
    print("ex%s %d: code %d, %d iterations, true residual %.2e" % (ex, etype, code, c.info.iterations, c.info.rel_resid))
    # W-3001 only where eps * kappa stands in the way: the second-order beams under pressure, body force and gravity
    assert code == 0 or (code == 3001 and (ex, etype) in UNCONFIRMED), (ex, etype, code)
    assert c.info.rel_resid <= 1.0e-8
    c.download_x(m)
    c.close()
    check_extrema(m.X, d["expect"])
