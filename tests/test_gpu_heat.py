"""Heat conduction assembly on the device (frontistr_amd/csrc/fx_heat.h, frontistr_amd/heat.py) against the numpy restatement
tests/heat_ref.py, which tests/test_heat_ref.py pins to the reference (its element routines, and fistr1's runs of the heat decks),
and against those runs themselves.

Shapes: the smallest skewed meshes of frontistr_amd.mesh on which the coloured scatter has more than one colour and a colour
with more elements than one workgroup holds, not a multiple of it -- HEAT_BS / HEAT_LPE elements, read from fx_heat.h.

Bounds: one element 1e-13 of the largest entry (the same sums in the same order: only the contraction of a * b + c differs);
assembled arrays 1e-12 of the largest entry, as the linear assembly tests (the colours add an entry's contributions in another
order).  Solution loops: the reference's own decks against what the unmodified fistr1 wrote for them (see there)."""
import functools
import os
import re

import numpy as np
import pytest

import heat_ref as R

pytestmark = pytest.mark.gpu

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "frontistr_amd", "csrc", "fx_heat.h")
TYPES = (341, 342, 351, 352, 361, 362)
COND3 = [(50.0, 0.0), (42.0, 200.0), (35.0, 500.0)]
CP2, RHO2 = [(0.46, 0.0), (0.52, 400.0)], [(7.85, 0.0), (7.70, 400.0)]
ROWS = [dict(cond=COND3, cp=CP2, rho=RHO2), dict(cond=[(20.0, 0.0)], cp=[(0.9, 100.0), (1.1, 300.0)], rho=[(2.7, 100.0), (2.6, 300.0)])]
SKEW, CURVE = 0.1, 0.03


def elements_per_workgroup():
    text = open(SRC).read()
    bs = int(re.search(r"#define HEAT_BS (\d+)", text).group(1))
    lpe = int(re.search(r"#define HEAT_LPE (\d+)", text).group(1))
    return bs // lpe


def _mesh(kind, n):
    from frontistr_amd.mesh import CubeMesh, MixedMesh, solid_mesh
    if kind == "mixed1":
        return MixedMesh(n, order=1, skew=SKEW)
    if kind == "mixed2":
        return MixedMesh(n, order=2, skew=SKEW, curve=CURVE)
    if kind == 361:
        return CubeMesh(n, skew=SKEW)
    return solid_mesh(n, kind, skew=SKEW, **({"curve": CURVE} if kind in (342, 352, 362) else {}))


def _groups(m):
    from frontistr_amd.mesh import mesh_groups
    return [(int(g[0]), np.asarray(g[1])) for g in mesh_groups(m)]


@functools.lru_cache(maxsize=None)
def case_mesh(kind):
    """the smallest n whose (first) group has several colours, one of them larger than a workgroup and not a multiple of it"""
    from frontistr_amd.mesh import color_elements
    epb = elements_per_workgroup()
    for n in range(2, 8):
        m = _mesh(kind, n)
        ok = False
        for et, conn in _groups(m):
            cnt = np.bincount(color_elements(conn, m.n_node))
            ok |= cnt.size > 1 and any(c > epb and c % epb for c in cnt)
        if ok:
            assert sum(c.shape[0] for _, c in _groups(m)) < 5000
            return m
    raise AssertionError("no mesh of %s reaches the shape" % (kind,))


def materials(hip_side):
    if hip_side:
        from frontistr_amd.heat import tHeatMaterial
        return [tHeatMaterial(**r) for r in ROWS]
    return [R.Material(**r) for r in ROWS]


def fields(coord):
    """temperatures over -100 .. 650: below the first row, inside both intervals, above the last row"""
    x = coord / np.abs(coord).max()
    temp = 275.0 + 375.0 * np.sin(3.1 * x[:, 0] + 1.3 * x[:, 1] - 2.2 * x[:, 2])
    temp0 = 250.0 + 300.0 * np.cos(2.3 * x[:, 0] - 1.1 * x[:, 1] + 0.7 * x[:, 2])
    return temp, temp0


@functools.lru_cache(maxsize=None)
def reference(kind, transient, variant=0):
    """(mesh, groups with material ids, restatement's Matrix) -- computed once, not changed by the tests"""
    m = case_mesh(kind)
    groups = [(et, conn, None, (1 + (np.arange(conn.shape[0]) % 2)).astype(np.int32)) for et, conn in _groups(m)]
    temp, temp0 = fields(m.coord)
    if variant:
        temp, temp0 = temp0 + 20.0, temp - 35.0
    A = R.profile_of(m.n_node, groups)
    beta, dtime = (0.5, 0.37) if transient else (1.0, 0.0)
    R.assemble(A, m.coord, groups, materials(False), temp, temp0, beta, dtime)
    return m, groups, A, temp, temp0, beta, dtime


def device_matrix(hip, A):
    from frontistr_amd.hecmw import hecmwST_matrix
    return hecmwST_matrix.from_arrays(A.NP, A.NP, A.indexL, A.itemL, A.indexU, A.itemU, np.zeros(A.NP), np.zeros(A.itemL.size),
                                      np.zeros(A.itemU.size), B=np.zeros(A.NP), X=np.zeros(A.NP), NDOF=1)


def assert_matches(M, A, tol=1e-12):
    big = max(np.abs(A.D).max(), np.abs(A.AL).max(), np.abs(A.AU).max())
    figures = {}
    for name in ("D", "AL", "AU"):
        figures[name] = np.abs(getattr(M, name) - getattr(A, name)).max() / big
    figures["B"] = np.abs(M.B - A.B).max() / max(np.abs(A.B).max(), 1e-300)
    print("relative differences:", {k: "%.2e" % v for k, v in figures.items()})
    for name, v in figures.items():
        assert v <= tol, (name, v)


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.SolverContext(device=0)
    yield c
    c.close()


# ---- one element -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("etype", TYPES)
def test_single_skewed_element(hip, ctx, etype):
    m = _mesh(etype, 2)
    nn = R.NODES[etype]
    rng = np.random.default_rng(etype)
    hmats, rmats = materials(True), materials(False)
    for k in range(4):
        X = m.coord[m.conn[(5 * k) % m.conn.shape[0]] - 1] + 0.02 * rng.standard_normal((nn, 3))
        # 0: every branch of the table (below, both intervals, above); 1: every point exactly on the breakpoint 200 (and 400 for
        # specific heat and density); 2: on the first row; 3: ntab == 1
        TT = [rng.uniform(-150.0, 700.0, nn), np.full(nn, 200.0), np.full(nn, 0.0), rng.uniform(-150.0, 700.0, nn)][k]
        T0 = [rng.uniform(-100.0, 600.0, nn), np.full(nn, 400.0), np.full(nn, 0.0), rng.uniform(0.0, 400.0, nn)][k]
        mi = 1 if k == 3 else 0
        ss, s0 = ctx.heat_element(etype, X, TT, hmats[mi], tt0=T0, dtime=0.25)
        SS = R.thermal(etype, X[None], TT[None], rmats[mi].cond)[0]
        S0 = R.capacity(etype, X[None], T0[None], rmats[mi].cp, rmats[mi].rho)[0]
        d1, d2 = np.abs(ss - SS).max() / np.abs(SS).max(), np.abs(s0 - S0).max() / np.abs(S0).max()
        print("TYPE=%d case %d: SS %.2e  S0 %.2e" % (etype, k, d1, d2))
        assert d1 <= 1e-13 and d2 <= 1e-13, (k, d1, d2)
        ss1, none = ctx.heat_element(etype, X, TT, hmats[mi])          # dtime = 0: no capacity term
        assert none is None and np.array_equal(ss1, ss)


# ---- assembled arrays ------------------------------------------------------------------------------------------------------------------
KINDS = TYPES + ("mixed1", "mixed2")


@pytest.mark.parametrize("transient", (False, True), ids=("steady", "transient"))
@pytest.mark.parametrize("kind", KINDS)
def test_assembled(hip, kind, transient):
    m, groups, A, temp, temp0, beta, dtime = reference(kind, transient)
    c = hip.SolverContext(device=0)
    try:
        M = device_matrix(hip, A)
        c.heat_assemble_groups(m.coord, groups, materials(True), M, temp, temp0, beta=beta, dtime=dtime)
        assert_matches(M, A)
        first = [a.copy() for a in (M.D, M.AL, M.AU, M.B)]
        s1 = c.heat_stats()
        assert s1["colourings"] == len(groups) and s1["maps"] == len(groups) and s1["profiles"] == 1
        for a in (M.D, M.AL, M.AU, M.B):
            a[:] = 7.0              # the call clears what it finds
        c.heat_assemble_groups(m.coord, groups, materials(True), M, temp, temp0, beta=beta, dtime=dtime)
        assert all(np.array_equal(a, b) for a, b in zip(first, (M.D, M.AL, M.AU, M.B))), "not bitwise reproducible"
        # new temperatures on the same context: nothing is coloured or mapped again
        _, _, A2, t2, t20, _, _ = reference(kind, transient, 1)
        c.heat_assemble_groups(m.coord, groups, materials(True), M, t2, t20, beta=beta, dtime=dtime)
        s2 = c.heat_stats()
        assert (s2["colourings"], s2["maps"], s2["profiles"]) == (s1["colourings"], s1["maps"], s1["profiles"]) and s2["calls"] == 3
        assert_matches(M, A2)
    finally:
        c.close()


def test_shapes_reach_the_scatter():
    """every case has several colours and a colour of more than one workgroup with a partly filled last one"""
    from frontistr_amd.mesh import color_elements
    epb = elements_per_workgroup()
    for kind in KINDS:
        m = case_mesh(kind)
        cnt = [np.bincount(color_elements(conn, m.n_node)) for _, conn in _groups(m)]
        assert any(c.size > 1 and any(v > epb and v % epb for v in c) for c in cnt), kind


def test_cflux_and_fixtemp_in_call(hip, ctx):
    import copy
    m, groups, A0, temp, temp0, beta, dtime = reference("mixed1", True)
    A = copy.deepcopy(A0)
    rng = np.random.default_rng(3)
    flux = np.where(rng.random(m.n_node) < 0.2, rng.uniform(-50.0, 50.0, m.n_node), 0.0)
    nodes = np.concatenate([m.bottom_nodes, m.top_nodes[::2]]).astype(np.int32)
    vals = np.concatenate([np.full(m.bottom_nodes.size, 20.0), np.linspace(300.0, 480.0, m.top_nodes[::2].size)])
    R.boundary(A, flux, (nodes, vals))
    M = device_matrix(hip, A)
    ctx.heat_assemble_groups(m.coord, groups, materials(True), M, temp, temp0, beta=beta, dtime=dtime, flux=flux, fix=(nodes, vals))
    assert_matches(M, A)
    assert np.array_equal(M.D[nodes - 1], np.ones(nodes.size)) and np.array_equal(M.B[nodes - 1], vals)


def test_errors_leave_the_arrays_untouched(hip, ctx):
    from frontistr_amd.heat import tHeatMaterial
    m, groups, A, temp, temp0, beta, dtime = reference(341, True)
    M = device_matrix(hip, A)
    for a in (M.D, M.AL, M.AU, M.B):
        a[:] = 3.25
    mats = materials(True)

    def refused(code, text, g=groups, ms=mats, mat=M, t=temp, t0=temp0, fix=None):
        with pytest.raises(hip.HecmwSolverError) as e:
            ctx.heat_assemble_groups(m.coord, g, ms, mat, t, t0, beta=beta, dtime=dtime, fix=fix)
        assert e.value.code == code and text in str(e.value), str(e.value)
        assert all(np.all(a == 3.25) for a in (M.D, M.AL, M.AU, M.B))

    conn, em = groups[0][1], groups[0][3]
    refused(-2, "not supported", g=[(331, conn, None, em)])
    M3 = device_matrix(hip, A)
    M3.NDOF = 3
    refused(-2, "NDOF", mat=M3)
    bad = conn.copy(); bad[5, 2] = m.n_node + 1
    refused(-1, "group 1, element 6: node id out of range", g=[(341, bad, None, em)])
    bad_em = em.copy(); bad_em[7] = 3
    refused(-1, "group 1, element 8: material id out of range", g=[(341, conn, None, bad_em)])
    twice = conn.copy(); twice[4, 3] = twice[4, 0]
    refused(-1, "group 1 (TYPE=341), element 5 names a node twice", g=[(341, twice, None, em)])
    broken = tHeatMaterial(**ROWS[0]); broken.cond = (0,) + broken.cond[1:]
    refused(-1, "ntab", ms=[broken, mats[1]])
    nocap = tHeatMaterial(cond=COND3)
    refused(-1, "ntab", ms=[nocap, mats[1]])                     # dtime > 0 reads specific heat and density
    refused(-1, "temp0 missing", t0=None)
    refused(-1, "fixed node id out of range", fix=(np.array([m.n_node + 1], dtype=np.int32), np.array([1.0])))
    refused(-1, "several materials need elem_mat", g=[(341, conn, None, None)])
    for member in ("D", "B", "indexL", "AL"):
        Mx = device_matrix(hip, A)
        setattr(Mx, member, None)
        refused(-1, "matrix arrays missing", mat=Mx)
    Mn = device_matrix(hip, A)
    Mn.NP += 1
    refused(-1, "mesh/profile size mismatch", mat=Mn)
    import ctypes as C                                            # no coordinates: through the C ABI itself
    tab, keep = ctx._group_table(groups)
    mt, keep_m, n_mat = ctx._heat_materials(mats)
    hv, mv = hip._HeatView(hip._ptr(temp), hip._ptr(temp0), beta, dtime), M.view()
    code = hip.lib().fx_heat_assemble_groups(ctx.h, m.n_node, None, len(groups), tab, n_mat, mt, C.byref(hv), C.byref(mv), None, 0, None,
                                             None, None)
    assert code == -1 and b"empty mesh" in hip.lib().fx_last_error() and all(np.all(a == 3.25) for a in (M.D, M.AL, M.AU, M.B))
    # a connectivity entry that the profile does not hold: two far nodes of the mesh in one element
    far = conn.copy(); far[0, 0] = conn[-1, 1] if conn[-1, 1] not in conn[0] else conn[-1, 2]
    assert far[0, 0] not in conn[0]
    refused(-1, "cannot find connectivity", g=[(341, far, None, em)])
    with pytest.raises(hip.HecmwSolverError) as e:                # 361 too: a collapsed hexahedron is refused here
        c8 = case_mesh(361)
        h = np.asarray(c8.conn).copy(); h[2, 7] = h[2, 6]
        A8 = R.profile_of(c8.n_node, [(361, h)])
        ctx.heat_assemble_groups(c8.coord, [(361, h)], mats[:1], device_matrix(hip, A8), np.zeros(c8.n_node), np.zeros(c8.n_node))
    assert e.value.code == -1 and "group 1 (TYPE=361), element 3 names a node twice" in str(e.value)
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.heat_element(331, np.zeros((4, 3)), np.zeros(4), mats[0])
    assert e.value.code == -2


# ---- the two loops on the reference's decks --------------------------------------------------------------------------------------------
# tests/golden/heat_decks.npz: what the unmodified fistr1 wrote for these decks (tests/golden/make_heat_golden.py).  The CPU test
# measures 9.8e-12 between the restatement (dense solve) and those files and bounds it by ten times that (DECK_BOUND); here the
# device CG stops at a relative residual of 1e-12 on another rounding path: ten times the CPU bound.
GPU_DECK_BOUND = 10 * 9.8e-11


def _deck_run(hip, ctx, name):
    import heat_decks as HD
    from conftest import load_golden
    from frontistr_amd.heat import heat_solve_SS, heat_solve_TRAN, tHeatMaterial
    d = HD.load(name)
    ids, temps, steps = HD.golden(load_golden("heat_decks"), name)
    assert np.array_equal(ids, d["ids"]) and d["interface"] is None
    mats = [tHeatMaterial(d["cond"], cp=d["cp"], rho=d["rho"])]
    kw = dict(fix=d["fix"], flux=d["flux"], eps=d["eps"], itmax=d["itmax"], resid=1e-12, maxit=10000, precond=1)
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


@pytest.mark.parametrize("name", ["N341", "N342", "N351", "N352", "N361", "N362", "O361"])
def test_heat_solve_SS_on_the_decks(hip, ctx, name):
    _deck_run(hip, ctx, name)


@pytest.mark.parametrize("name", ["N361T", "N342T"])
def test_heat_solve_TRAN_on_the_decks(hip, ctx, name):
    _deck_run(hip, ctx, name)


def test_automatic_time_step_is_refused(hip, ctx):
    from frontistr_amd.heat import heat_solve_TRAN
    m = _mesh(361, 2)
    with pytest.raises(NotImplementedError):
        heat_solve_TRAN(ctx, m.coord, [(361, m.conn, None, None)], materials(True)[:1], np.zeros(m.n_node), 0.4, 1.5, delmin=0.01)
