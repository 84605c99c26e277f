"""The surface terms of a heat analysis on the device (frontistr_amd/csrc/fx_heat_bc.h, frontistr_amd/heat.py) against the numpy
restatement tests/heat_bc_ref.py, which tests/test_heat_bc_ref.py pins to the reference (its face routines bit for bit, and
fistr1's runs of the exP, exQ, exR, exS decks), and against those runs themselves.

Shapes: per kind of mesh the smallest skewed mesh of frontistr_amd.mesh whose boundary faces -- all six sides, which is where the
lists of this file put !DFLUX, !FILM and !RADIATE -- make a list (per group and face shape, as the device keeps them) with several
colours, one of them holding more faces than one workgroup (HEATF_BS / HEATF_LPF, read from fx_heat_bc.h) and not a multiple of
it; under 5000 elements.  The wedge meshes carry triangles and quadrilaterals together.  The body flux lies on every second element.

Bounds: one face 1e-13 of the largest entry (the same sums in the same order, the face kernel compiled without
contraction: measured 5.3e-16); assembled arrays 1e-12 of the largest entry (the colours add an entry's contributions in another order than the
list).  Decks: ten times the CPU bound of test_heat_bc_ref.py, the ratio test_gpu_heat.py uses."""
import copy
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import heat_bc_ref as B
import heat_ref as R
import test_gpu_heat as TG
from conftest import load_golden

pytestmark = pytest.mark.gpu

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "frontistr_amd", "csrc", "fx_heat_bc.h")
TYPES = TG.TYPES
KINDS = TG.KINDS
TZERO = 100.0                     # inside the temperatures of TG.fields: TT - TZERO takes both signs
GPU_DECK_BOUND = 10 * 4.3e-11     # test_heat_bc_ref.DECK_BOUND


def faces_per_workgroup():
    text = open(SRC).read()
    return int(re.search(r"#define HEATF_BS (\d+)", text).group(1)) // int(re.search(r"#define HEATF_LPF (\d+)", text).group(1))


def boundary_faces(groups):
    """(group, elem, face) of every face that one element alone has, in group, element, face order"""
    seen = {}
    for g, grp in enumerate(groups):
        et, conn = int(grp[0]), np.asarray(grp[1])
        for f in range(1, B.NFACE[et] + 1):
            nod = B.face_nodes(et, f)
            ncorner = 3 if len(nod) in (3, 6) else 4
            keys = np.sort(conn[:, nod[:ncorner]], axis=1)
            for e, k in enumerate(map(tuple, keys)):
                seen.setdefault(k, []).append((g, e, f))
    out = sorted(v[0] for v in seen.values() if len(v) == 1)
    return tuple(np.array(c, dtype=np.int32) for c in zip(*out))


def face_lists(groups, g, e, f):
    """the face connectivities as the device keeps them: {(group, nodes per face): (n, mm) node ids}"""
    out = {}
    for gi, ei, fi in zip(g, e, f):
        et, conn = int(groups[gi][0]), np.asarray(groups[gi][1])
        nod = B.face_nodes(et, fi)
        out.setdefault((gi, len(nod) % 3 == 0), []).append(conn[ei, nod])
    return {k: np.array(v) for k, v in out.items()}


def _reaches(m, groups):
    from frontistr_amd.mesh import color_elements
    fpb = faces_per_workgroup()
    for fc in face_lists(groups, *boundary_faces(groups)).values():
        cnt = np.bincount(color_elements(np.ascontiguousarray(fc, dtype=np.int32), m.n_node))
        if cnt.size > 1 and any(c > fpb and c % fpb for c in cnt):
            return True
    return False


@functools.lru_cache(maxsize=None)
def case_mesh(kind):
    for n in range(2, 9):
        m = TG._mesh(kind, n)
        groups = TG._groups(m)
        if _reaches(m, groups):
            assert sum(c.shape[0] for _, c in groups) < 5000
            return m
    raise AssertionError("no mesh of %s reaches the shape" % (kind,))


def lists_of(m, groups, repeat=False):
    """dflux on every boundary face and BF on every second element, film and radiate on every boundary face; values vary per entry.
    repeat: the film list names 10 % of its entries a second time"""
    g, e, f = boundary_faces(groups)
    n = g.size
    k = np.arange(n)
    conns = [np.asarray(grp[1]) for grp in groups]
    bg = np.concatenate([np.full(len(range(0, c.shape[0], 2)), gi, dtype=np.int32) for gi, c in enumerate(conns)])
    be = np.concatenate([np.arange(0, c.shape[0], 2, dtype=np.int32) for c in conns])
    dflux = (np.concatenate([g, bg]), np.concatenate([e, be]), np.concatenate([f, np.zeros(bg.size, dtype=np.int32)]),
             np.concatenate([2500.0 + 10.0 * (k % 7), 900.0 - 3.0 * (np.arange(bg.size) % 11)]))
    film = (g, e, f, 25.0 + 0.5 * (k % 5), 600.0 - 20.0 * (k % 3))
    if repeat:
        again = k[::10]
        film = tuple(np.concatenate([a, a[again]]) for a in film)
    radiate = (g, e, f, np.full(n, 1.1164e-8) * (1.0 + 0.1 * (k % 4)), 500.0 + 30.0 * (k % 2))
    return dflux, film, radiate


@functools.lru_cache(maxsize=None)
def reference(kind, transient, variant=0, repeat=False):
    """(mesh, groups with material ids, restatement's Matrix with the surface terms, ...) -- computed once, not changed by the tests"""
    m = case_mesh(kind)
    groups = [(et, conn, None, (1 + (np.arange(conn.shape[0]) % 2)).astype(np.int32)) for et, conn in TG._groups(m)]
    temp, temp0 = TG.fields(m.coord)
    if variant:
        temp, temp0 = temp0 + 20.0, temp - 35.0
    A = R.profile_of(m.n_node, groups)
    beta, dtime = (0.5, 0.37) if transient else (1.0, 0.0)
    R.assemble(A, m.coord, groups, TG.materials(False), temp, temp0, beta, dtime)
    A0 = copy.deepcopy(A)
    lists = lists_of(m, groups, repeat)
    B.surface_terms(A, m.coord, groups, temp, *lists, tzero=TZERO)
    return m, groups, A, temp, temp0, beta, dtime, lists, A0


def call(c, ref, M, temp=None, temp0=None, **kw):
    m, groups, _, t, t0, beta, dtime, lists, _ = ref
    args = dict(dflux=lists[0], film=lists[1], radiate=lists[2], tzero=TZERO)
    args.update(kw)
    return c.heat_assemble_groups(m.coord, groups, TG.materials(True), M, t if temp is None else temp, t0 if temp0 is None else temp0,
                                  beta=beta, dtime=dtime, **args)


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.SolverContext(device=0)
    yield c
    c.close()


# ---- one face --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("etype", TYPES)
def test_single_faces_against_the_reference_routines(hip, ctx, etype):
    g = load_golden("heat_faces")
    HH, SINK, RR, Q = (float(v) for v in g["vals"])
    worst, n = 0.0, 0
    for k in range(int(g["n"])):
        if int(g["etype%d" % k]) != etype:
            continue
        X, TT, tz = g["X%d" % k], g["TT%d" % k], float(g["tzero%d" % k])
        for face in range(B.NFACE[etype] + 1):
            _, v, nod = ctx.heat_face(etype, "dflux", face, X, Q)
            ref = g["dflux%d_%d" % (k, face)]
            worst = max(worst, np.abs(v - ref).max() / np.abs(ref).max())
            if face == 0:
                assert nod.tolist() == list(range(1, R.NODES[etype] + 1))
                continue
            for kind, val, tt in (("film", HH, None), ("radiate", RR, TT)):
                t1, t2, nod = ctx.heat_face(etype, kind, face, X, val, sink=SINK, tt=tt, tzero=tz)
                assert np.array_equal(nod, g["nod%d_%d" % (k, face)])
                r1, r2 = g["%s1_%d_%d" % (kind, k, face)], g["%s2_%d_%d" % (kind, k, face)]
                worst = max(worst, np.abs(t1 - r1).max() / np.abs(r1).max(), np.abs(t2 - r2).max() / np.abs(r2).max())
                n += 1
    print("TYPE=%d: %d faces of film and radiate, dflux and BF: largest relative difference %.2e" % (etype, n, worst))
    assert n == 2 * 3 * B.NFACE[etype] and worst <= 1e-13, worst


# ---- assembled arrays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transient", (False, True), ids=("steady", "transient"))
@pytest.mark.parametrize("kind", KINDS)
def test_assembled(hip, kind, transient):
    ref = reference(kind, transient)
    m, groups, A = ref[:3]
    c = hip.SolverContext(device=0)
    try:
        M = TG.device_matrix(hip, A)
        call(c, ref, M)
        TG.assert_matches(M, A)
        first = [a.copy() for a in (M.D, M.AL, M.AU, M.B)]
        s1, b1 = c.heat_stats(), c.heat_bc_stats()
        nlist = len(face_lists(groups, *boundary_faces(groups)))
        # per group and shape: one list each of dflux, film, radiate (colourings), a map for film and radiate; BF: one list per group
        assert b1["face_colourings"] == 3 * nlist + len(groups) and b1["face_maps"] == 2 * nlist and s1["colourings"] == len(groups)
        for a in (M.D, M.AL, M.AU, M.B):
            a[:] = 7.0
        call(c, ref, M)
        assert all(np.array_equal(a, b) for a, b in zip(first, (M.D, M.AL, M.AU, M.B))), "not bitwise reproducible"
        # the entry point without surface terms in between, then new temperatures: nothing is coloured or mapped again
        M0 = TG.device_matrix(hip, A)
        c.heat_assemble_groups(m.coord, groups, TG.materials(True), M0, ref[3], ref[4], beta=ref[5], dtime=ref[6])
        TG.assert_matches(M0, ref[8])
        ref2 = reference(kind, transient, 1)
        call(c, ref, M, temp=ref2[3], temp0=ref2[4])
        s2, b2 = c.heat_stats(), c.heat_bc_stats()
        assert (b2["face_colourings"], b2["face_maps"]) == (b1["face_colourings"], b1["face_maps"])
        assert (s2["colourings"], s2["maps"], s2["profiles"]) == (s1["colourings"], s1["maps"], s1["profiles"]) and s2["calls"] == 4
        TG.assert_matches(M, ref2[2])
    finally:
        c.close()


def test_shapes_reach_the_scatter():
    fpb = faces_per_workgroup()
    assert fpb == 8
    for kind in KINDS:
        m = case_mesh(kind)
        assert _reaches(m, TG._groups(m)), kind
    for kind in (351, 352, "mixed1", "mixed2"):
        groups = TG._groups(case_mesh(kind))
        g, e, f = boundary_faces(groups)
        mm = set(len(B.face_nodes(int(groups[gi][0]), fi)) for gi, fi in zip(g, f) if int(groups[gi][0]) in (351, 352))
        assert mm in ({3, 4}, {6, 8}), (kind, mm)             # triangles and quadrilaterals together


@pytest.mark.parametrize("kind", (361, 352))
def test_repeated_entries_add_twice(hip, ctx, kind):
    ref = reference(kind, False, 0, True)
    once = reference(kind, False)
    assert ref[7][1][0].size > once[7][1][0].size and np.abs(ref[2].D - once[2].D).max() > 0
    M = TG.device_matrix(hip, ref[2])
    call(ctx, ref, M)
    TG.assert_matches(M, ref[2])


def test_without_lists_the_arrays_are_those_of_the_old_entry_point(hip, ctx):
    ref = reference("mixed2", True)
    m, groups, _, temp, temp0, beta, dtime = ref[:7]
    mats = TG.materials(True)
    M1, M2, M3 = (TG.device_matrix(hip, ref[2]) for _ in range(3))
    ctx.heat_assemble_groups(m.coord, groups, mats, M1, temp, temp0, beta=beta, dtime=dtime, dflux=None, film=None, radiate=None)
    tab, keep = ctx._group_table(groups)
    mt, keep_m, n_mat = ctx._heat_materials(mats)
    coord = np.ascontiguousarray(m.coord, dtype=np.float64)
    hv = hip._HeatView(hip._ptr(temp), hip._ptr(temp0), beta, dtime)
    mv2, mv3 = M2.view(), M3.view()
    assert hip.lib().fx_heat_assemble_groups(ctx.h, m.n_node, hip._ptr(coord), len(groups), tab, n_mat, mt, C.byref(hv), C.byref(mv2), None, 0,
                                             None, None, None) == 0
    empty = hip._HeatBc()
    assert hip.lib().fx_heat_assemble_groups_bc(ctx.h, m.n_node, hip._ptr(coord), len(groups), tab, n_mat, mt, C.byref(hv), C.byref(mv3), None, 0,
                                                None, None, C.byref(empty), None) == 0
    for name in ("D", "AL", "AU", "B"):
        assert np.array_equal(getattr(M1, name), getattr(M2, name)) and np.array_equal(getattr(M3, name), getattr(M2, name)), name
    TG.assert_matches(M2, ref[8])
    assert hip.lib().fx_heat_assemble_groups_bc(ctx.h, m.n_node, hip._ptr(coord), len(groups), tab, n_mat, mt, C.byref(hv), C.byref(mv3), None, 0,
                                                None, None, None, None) == -1


def test_refusals_leave_the_arrays_untouched(hip, ctx):
    m361, m341 = TG._mesh(361, 2), TG._mesh(341, 2)
    for m, et, bad_face in ((m361, 361, 7), (m341, 341, 5)):
        groups = [(et, np.asarray(m.conn), None, None)]
        A = R.profile_of(m.n_node, groups)
        M = TG.device_matrix(hip, A)
        for a in (M.D, M.AL, M.AU, M.B):
            a[:] = 3.25
        temp = np.full(m.n_node, 300.0)
        i0 = np.zeros(1, dtype=np.int32)

        def refused(text, **kw):
            with pytest.raises(hip.HecmwSolverError) as e:
                ctx.heat_assemble_groups(m.coord, groups, TG.materials(True)[:1], M, temp, temp, **kw)
            assert e.value.code == -1 and text in str(e.value), str(e.value)
            assert all(np.all(a == 3.25) for a in (M.D, M.AL, M.AU, M.B))

        refused("film, entry 1: TYPE=%d has no face 0" % et, film=(i0, i0, i0, 25.0, 600.0))
        refused("has no face %d" % bad_face, dflux=(i0, i0, i0 + bad_face, 1.0))
        refused("has no face %d" % bad_face, radiate=(i0, i0, i0 + bad_face, 1e-8, 600.0))
        refused("is not in group 1", film=(i0, i0 + m.conn.shape[0], i0 + 1, 25.0, 600.0))
        refused("group out of range", dflux=(i0 + 1, i0, i0 + 1, 1.0))
        refused("radiate: list arrays missing", radiate=(i0, i0, i0 + 1, 1e-8, None))
        ctx.heat_assemble_groups(m.coord, groups, TG.materials(True)[:1], M, temp, temp, dflux=(i0, i0, i0, 1.0))     # BF is face 0 of dflux
        assert not np.any(M.D == 3.25)
    with pytest.raises(hip.HecmwSolverError):
        ctx.heat_face(361, "film", 0, np.zeros((8, 3)), 1.0)
    with pytest.raises(hip.HecmwSolverError):
        ctx.heat_face(361, "radiate", 1, np.zeros((8, 3)), 1.0)          # no temperatures


# ---- the two loops on the reference's decks --------------------------------------------------------------------------------------------
def _deck_run(hip, ctx, name):
    import heat_bc_decks as BD
    from frontistr_amd.heat import heat_solve_SS, heat_solve_TRAN, tHeatAmplitude, tHeatMaterial
    d = BD.load(name, amplitude=tHeatAmplitude)
    ids, temps, steps = BD.golden(load_golden("heat_bc_decks"), name)
    assert np.array_equal(ids, d["ids"])
    mats = [tHeatMaterial(d["cond"], cp=d["cp"], rho=d["rho"])]
    kw = dict(fix=d["fix"], flux=d["flux"], dflux=d["dflux"], film=d["film"], radiate=d["radiate"], tzero=d["zero"], eps=d["eps"],
              itmax=d["itmax"], resid=1e-12, maxit=10000, precond=1)
    if d["dt"] > 0:
        got = []
        t, st, times = heat_solve_TRAN(ctx, d["coord"], d["groups"], mats, d["temp0"], d["dt"], d["etime"], delmin=d["dtmin"], keep=got, **kw)
    else:
        t, h = heat_solve_SS(ctx, d["coord"], d["groups"], mats, d["temp0"], **kw)
        st, got = [h], [t]
    assert len(got) == temps.shape[0]
    diff = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(got, temps))
    print("%s: iterALL per step %s (fistr1 %s), largest relative difference %.2e" % (name, [len(x) for x in st], [len(x) for x in steps], diff))
    assert [len(x) for x in st] == [len(x) for x in steps]
    assert diff <= GPU_DECK_BOUND, diff


@pytest.mark.parametrize("name", ["%s%d" % (d, t) for d in "PQRS" for t in TYPES])
def test_heat_solve_SS_on_the_decks(hip, ctx, name):
    _deck_run(hip, ctx, name)


@pytest.mark.parametrize("name", ["S361T", "S352T"])
def test_heat_solve_TRAN_on_the_decks(hip, ctx, name):
    _deck_run(hip, ctx, name)
