"""fstr_NodalStress3D on the device (csrc/fx_nodal_stress.h: fx_nodal_stress_groups, fx_nl_nodal_stress) through
frontistr_amd/hecmw.py and fstr.py against the numpy restatement tests/nodal_stress_ref.py.

The pass reads connectivity and quadrature-point values only, so the inputs are small meshes that can be enumerated and point
values that are random, seeded and O(1) (no cancellation hides an error): a 3^3-cell block of each of the six types (node valences
1, 2, 4, 8), an 8^3-cell block (more nodes than two 256-lane workgroups of the node kernel, more elements than two workgroups of the
element kernel: 21 elements each, 10 at 362 -- read back from the library), a fan of tetrahedra around a hub, mixed meshes whose
interface nodes belong to groups of different types, a node that no element names, a collapsed hexahedron, two groups of one type.

Bound: ten times the deviation of the restatement from the reference program, measured on the CPU by
tests/golden/make_nodal_stress_golden.py and asserted by tests/test_nodal_stress_ref.py.  That deviation is 0 on every recorded
array (17 digits in the result files; the restatement repeats the reference's operations in its order), so the bound is 0: the
device arrays equal the restatement's bit for bit.  Every comparison prints its largest deviation before it asserts.

One test holds the device against the reference program itself: the point arrays the unmodified program wrote for the nine recorded
decks go in, and the arrays the same run wrote are what must come out."""
import ctypes as C

import numpy as np
import pytest

import nodal_stress_ref as NR

pytestmark = pytest.mark.gpu
FX_ERROR_RUNTIME, FX_ERROR_UNSUPPORTED = -1, -2
BOUND = NR.BOUND
ALL = NR.ALL
ARRAYS = ("strain", "stress", "mises", "estrain", "estress", "emises", "pstress", "pstress_vect", "pstrain", "pstrain_vect",
          "epstress", "epstress_vect", "epstrain", "epstrain_vect")
FLAG_OF = {"pstress": 1, "pstress_vect": 2, "pstrain": 4, "pstrain_vect": 8, "epstress": 16, "epstress_vect": 32, "epstrain": 64,
           "epstrain_vect": 128}


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.SolverContext()
    yield c
    c.close()


def points(groups, seed):
    """seeded O(1) point values per group: (strain list, stress list), stress on another scale than strain"""
    rng = np.random.default_rng(seed)
    st = [rng.uniform(-1.0, 1.0, (np.asarray(g[1]).shape[0], NR.NQ[g[0]], 6)) for g in groups]
    ss = [rng.uniform(-3.0, 3.0, (np.asarray(g[1]).shape[0], NR.NQ[g[0]], 6)) for g in groups]
    return st, ss


def block(etype, n):
    from frontistr_amd.mesh import CubeMesh, solid_mesh
    m = CubeMesh(n) if etype == 361 else solid_mesh(n, etype)
    return m.n_node, [(etype, m.conn)]


def second_order(conn, etype):
    """mid-edge nodes for a first-order connectivity, one per edge, in the node order of `etype`"""
    conn = np.asarray(conn)
    ids, out, nxt = {}, [], int(conn.max()) + 1
    for row in conn:
        extra = []
        for a, b in NR.PAIRS[etype]:
            key = (min(row[a], row[b]), max(row[a], row[b]))
            if key not in ids:
                ids[key] = nxt
                nxt += 1
            extra.append(ids[key])
        out.append(list(row) + extra)
    return nxt - 1, np.array(out, dtype=np.int32)


def fan(etype, k=24):
    """k tetrahedra around the edge hub - top: both are held by k elements, each ring node by two"""
    conn = np.array([[1, 3 + i, 3 + (i + 1) % k, 2] for i in range(k)], dtype=np.int32)
    if etype == 341:
        return k + 2, [(341, conn)]
    n_node, c = second_order(conn, 342)
    return n_node, [(342, c)]


def compare(res, ref, flags=ALL, tag=""):
    worst = {}
    for name in ARRAYS:
        got, want = getattr(res, name), getattr(ref, name)
        if name in FLAG_OF and not flags & FLAG_OF[name]:
            assert got is None, name
            continue
        assert got is not None and got.shape == want.shape, name
        scale = np.abs(want).max()
        worst[name] = float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max())
    print(tag, "largest deviation from the restatement, relative to the array's largest magnitude:", worst)
    assert max(worst.values()) <= BOUND, worst


def run_case(ctx, n_node, groups, seed, flags=ALL, tag=""):
    st, ss = points(groups, seed)
    res = ctx.nodal_stress_groups(n_node, groups, st, ss, principal=flags)
    ref = NR.nodal_stress(n_node, groups, st, ss, principal=flags)
    assert not ref.failed
    assert res.n_node == n_node and res.n_elem == sum(np.asarray(g[1]).shape[0] for g in groups)
    compare(res, ref, flags, tag)
    return res, ref


@pytest.mark.parametrize("etype", [341, 342, 351, 352, 361, 362])
def test_block_of_27_cells(ctx, etype):
    n_node, groups = block(etype, 3)
    _, ref = run_case(ctx, n_node, groups, etype, tag="%d 3^3" % etype)
    if etype == 361:
        assert sorted(set(ref.count.tolist())) == [1, 2, 4, 8]


@pytest.mark.parametrize("etype", [341, 342, 351, 352, 361, 362])
def test_more_than_two_workgroups_of_each_kernel(ctx, etype):
    n_node, groups = block(etype, 8)
    s = ctx.nodal_stats()
    assert n_node > 2 * s["node_bs"] and groups[0][1].shape[0] > 2 * s["elems_per_wg"][etype]
    assert groups[0][1].shape[0] % s["elems_per_wg"][etype] != 0      # a partly filled last workgroup
    run_case(ctx, n_node, groups, 100 + etype, tag="%d 8^3" % etype)


@pytest.mark.parametrize("etype", [341, 342])
def test_fan_with_a_hub(ctx, etype):
    n_node, groups = fan(etype)
    _, ref = run_case(ctx, n_node, groups, 200 + etype, tag="%d fan" % etype)
    assert ref.count[0] == 24 and ref.count[1] == 24


@pytest.mark.parametrize("order,n", [(1, 2), (2, 2), (1, 4), (2, 3)])
def test_mixed_mesh(ctx, order, n):
    from frontistr_amd.mesh import MixedMesh
    m = MixedMesh(n, order=order)
    groups = [(g[0], g[1]) for g in m.groups]
    assert [g[0] for g in groups] == ([361, 351, 341] if order == 1 else [362, 352, 342])
    held = [set(np.unique(g[1]).tolist()) for g in groups]
    assert held[0] & held[1] and held[1] & held[2]          # interface nodes shared by groups of different types
    run_case(ctx, m.n_node, groups, 300 + 10 * order + n, tag="mixed order %d n %d" % (order, n))


def test_a_node_no_element_names(ctx):
    n_node, groups = block(361, 2)
    conn = groups[0][1].copy()
    conn[conn >= 14] += 1               # id 14 is free now, and two more ids past the end
    res, ref = run_case(ctx, n_node + 3, [(361, conn)], 41, tag="unnamed nodes")
    for i in (13, n_node + 1, n_node + 2):
        assert ref.count[i] == 0
        assert not res.strain[i].any() and not res.stress[i].any() and res.mises[i] == 0.0
        assert not res.pstress[i].any() and not res.pstress_vect[i].any() and not res.pstrain_vect[i].any()


def test_a_collapsed_hexahedron(ctx):
    n_node, groups = block(361, 2)
    conn = groups[0][1].copy()
    conn[3, 7] = conn[3, 6]             # names a node twice: added and counted twice
    _, ref = run_case(ctx, n_node, [(361, conn)], 42, tag="collapsed")
    assert ref.count[conn[3, 6] - 1] == np.count_nonzero(conn == conn[3, 6])


@pytest.mark.parametrize("etype", [361, 342])
def test_two_groups_of_one_type(ctx, etype):
    """against the restatement, and the nodal arrays bit for bit those of the same elements in one group"""
    n_node, groups = block(etype, 3)
    conn = groups[0][1]
    cut = conn.shape[0] // 3 + 1
    two = [(etype, conn[:cut]), (etype, conn[cut:])]
    res2, _ = run_case(ctx, n_node, two, 50 + etype, tag="two groups")
    st, ss = points(two, 50 + etype)
    res1 = ctx.nodal_stress_groups(n_node, groups, [np.concatenate(st)], [np.concatenate(ss)], principal=ALL)
    for name in ARRAYS:
        assert getattr(res1, name).tobytes() == getattr(res2, name).tobytes(), name


def test_two_calls_give_identical_bytes_and_one_list(ctx):
    n_node, groups = block(352, 3)
    st, ss = points(groups, 60)
    before = ctx.nodal_stats()["lists"]
    a = ctx.nodal_stress_groups(n_node, groups, st, ss, principal=ALL)
    b = ctx.nodal_stress_groups(n_node, groups, st, ss, principal=ALL)
    for name in ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    s = ctx.nodal_stats()
    assert s["lists"] == before + 1                                # built once, kept with the context
    assert s["entries"] == groups[0][1].size and s["records"] == 6 * groups[0][1].shape[0]
    n2, g2 = block(351, 3)                                          # another mesh: another list
    ctx.nodal_stress_groups(n2, g2, *points(g2, 61))
    assert ctx.nodal_stats()["lists"] == before + 2


@pytest.mark.parametrize("flags", [0, 1, 2, 4, 8, 16, 32, 64, 128, ALL])
def test_principal_flags(ctx, flags):
    from frontistr_amd.mesh import MixedMesh
    m = MixedMesh(2, order=2)
    run_case(ctx, m.n_node, [(g[0], g[1]) for g in m.groups], 70, flags=flags, tag="flags %d" % flags)


def test_degenerate_tensors(ctx):
    """single-point tetrahedra with nodes of their own: element and nodal tensors ARE the point values.  A diagonal tensor, one
    whose off-diagonal terms sum to less than eigen3's 1e-10, two equal values, the zero tensor, a full tensor with a double root."""
    t = np.array([[3.0, 1.0, 2.0, 0.0, 0.0, 0.0],
                  [1.0, 2.0, 3.0, 1e-11, -2e-11, 3e-11],
                  [2.0, 2.0, 5.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [1.0, 1.0, 1.0, 0.5, 0.5, 0.5],
                  [-4.0, 7.0, 0.5, 1.5, -2.5, 0.25]])
    conn = (1 + np.arange(4 * t.shape[0], dtype=np.int32)).reshape(-1, 4)
    groups = [(341, conn)]
    st, ss = [t[:, None, :].copy()], [t[::-1, None, :].copy()]
    res = ctx.nodal_stress_groups(conn.size, groups, st, ss, principal=ALL)
    ref = NR.nodal_stress(conn.size, groups, st, ss, principal=ALL)
    compare(res, ref, ALL, "degenerate tensors")
    assert np.array_equal(res.epstrain[0], [3.0, 2.0, 1.0]) and np.array_equal(res.epstrain[1], [3.0, 2.0, 1.0])
    assert np.array_equal(res.epstrain[2], [5.0, 2.0, 2.0]) and not res.epstrain_vect[3].any()
    assert np.array_equal(res.epstrain_vect[0], [[3.0, 0, 0], [0, 0, 2.0], [0, 1.0, 0]])


def test_errors_leave_the_outputs_untouched(ctx, hip):
    n_node, groups = block(361, 2)
    conn = groups[0][1]
    st, ss = points(groups, 80)
    lib = hip.lib()

    def call(n_node, etype, c, flags=0):
        tab, keep = hip.SolverContext._group_table([(etype, c)])
        tab[0].n_elem = c.shape[0]
        res, ms = hip._NodalResult(), C.c_float(-1.0)
        res.n_node, res.n_elem = -7, -7
        a, b = np.ascontiguousarray(st[0]), np.ascontiguousarray(ss[0])
        code = lib.fx_nodal_stress_groups(ctx.h, n_node, 1, tab, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), flags,
                                          C.byref(res), C.byref(ms))
        untouched = res.n_node == -7 and res.n_elem == -7 and not res.strain and not res.mises and ms.value == -1.0
        return code, untouched, lib.fx_last_error().decode()
    assert call(n_node, 361, conn)[:2] == (0, False)
    code, untouched, msg = call(n_node, 301, conn)
    assert code == FX_ERROR_UNSUPPORTED and untouched and "301" in msg
    bad = conn.copy()
    bad[5, 2] = n_node + 1
    code, untouched, msg = call(n_node, 361, bad)
    assert code == FX_ERROR_RUNTIME and untouched and "element 6" in msg
    bad[5, 2] = 0
    assert call(n_node, 361, bad)[:2] == (FX_ERROR_RUNTIME, True)
    assert call(n_node, 361, conn, flags=256)[:2] == (FX_ERROR_RUNTIME, True)
    # a connectivity with the wrong number of nodes per element, through the Python layer (fx_elem_group carries no row length)
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.nodal_stress_groups(n_node, [(342, conn)], st, ss)
    assert e.value.code == FX_ERROR_UNSUPPORTED
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.nodal_stress_groups(n_node, [(361, bad)], st, ss)
    assert e.value.code == FX_ERROR_RUNTIME
    run_case(ctx, n_node, groups, 81, tag="after the refusals")     # the context still serves


@pytest.mark.parametrize("name", ["B341", "B342", "B351", "B352", "B361", "B362", "hexpritet", "C3D8beam", "necking"])
def test_recorded_point_arrays_against_the_recorded_results(ctx, name):
    """The device against the reference program itself: the ISTRAIN / ISTRESS the unmodified program wrote go through
    fx_nodal_stress_groups, and what comes back is held against the arrays the same run wrote (tests/golden/nodal_stress*.npz)
    -- six single-type linear decks, the 361 + 351 + 341 mesh (addition across groups of different types), two nonlinear decks.
    Bound as above: 0.  Vectors where the recorded values are separated, up to the sign of a column."""
    import nodal_stress_decks as ND
    g = np.load(ND.golden_file(name))
    a = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_")}
    ids, groups, _ = ND.load(name)
    res = ctx.nodal_stress_groups(ids.size, groups, a["ISTRAIN"].ravel(), a["ISTRESS"].ravel(), principal=1 | 2 | 4 | 16 | 32)
    worst = {}
    for key, got in (("NSTRAIN", res.strain), ("NSTRESS", res.stress), ("NMISES", res.mises), ("ESTRAIN", res.estrain),
                     ("ESTRESS", res.estress), ("EMISES", res.emises), ("PRINC_NSTRESS", res.pstress),
                     ("PRINC_NSTRAIN", res.pstrain), ("PRINC_ESTRESS", res.epstress)):
        worst[key] = float(np.abs(got - a[key]).max() / np.abs(a[key]).max())
    for key, vals, got in (("PRINCV_NSTRESS", a["PRINC_NSTRESS"], res.pstress_vect), ("PRINCV_ESTRESS", a["PRINC_ESTRESS"], res.epstress_vect)):
        s = 1e-6 * np.abs(vals).max()
        ok = (np.abs(vals[:, 0] - vals[:, 1]) > s) & (np.abs(vals[:, 1] - vals[:, 2]) > s) & (np.abs(vals[:, 0] - vals[:, 2]) > s)
        if ok.any():
            sign = np.sign(np.einsum("njc,njc->nj", got[ok], a[key][ok]))[:, :, None]
            worst[key] = float(np.abs(got[ok] * sign - a[key][ok]).max() / np.abs(a[key]).max())
    print(name, "largest deviation from the recorded arrays, relative to the array's largest magnitude:", worst)
    assert max(worst.values()) <= BOUND, worst


def test_a_flat_connectivity_is_taken_as_assemble_groups_takes_it(ctx):
    n_node, groups = block(352, 3)
    st, ss = points(groups, 90)
    a = ctx.nodal_stress_groups(n_node, groups, st, ss)
    b = ctx.nodal_stress_groups(n_node, [(352, groups[0][1].ravel())], st, ss)
    assert a.stress.tobytes() == b.stress.tobytes() and a.emises.tobytes() == b.emises.tobytes()


# ---- the resident state of a nonlinear context -------------------------------------------------------------------------------
E0, NU0 = 206900.0, 0.29


def _newton(hip, coord, groups, mats, bc, nsub=3, elemopt=None):
    """a few Newton sub-steps of a small plastic mesh -> (ctx, solid)"""
    from frontistr_amd import fstr
    from oracle.refrun import default_params
    hm = hip.hecmwST_local_mesh(n_node=coord.shape[0])
    hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
    c = hip.SolverContext()
    c.upload(hecMAT, what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(c, coord, None, mats, groups=groups)
    hecMAT.Iarray[:], hecMAT.Rarray[:] = default_params(method=1, precond=1, maxit=5000, tol=1e-12)
    for sub in range(1, nsub + 1):      # the state is committed whether or not CONVERG was reached: the pass reads what is resident
        fstr.fstr_Newton(solid, hecMAT, ((sub - 1) / nsub, sub / nsub), bc, None, 30, 1e-3, commit_unconverged=True)
    return c, solid


def _stretch(m):
    node, dof, val = m.dirichlet()
    t = m.top_nodes
    return (np.concatenate([node, t, t]).astype(np.int32), np.concatenate([dof, np.full(t.size, 3), np.full(t.size, 1)]).astype(np.int32),
            np.concatenate([val, np.full(t.size, 0.004 * m.n), np.full(t.size, 0.001 * m.n)]))


def _nl_case(name):
    from frontistr_amd import fstr
    from frontistr_amd.mesh import CubeMesh, MixedMesh
    mises = lambda flag: fstr.tMaterial(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom_flag=flag)
    if name == "bbar":
        m = CubeMesh(3, skew=0.05)
        return m, [(361, m.conn, 2, None)], [mises(fstr.UPDATELAG)]
    if name == "fbar":
        m = CubeMesh(3, skew=0.05)
        return m, [(361, m.conn, 4, None)], [mises(fstr.TOTALLAG)]
    m = MixedMesh(2, order=2 if name == "mixed2" else 1, skew=0.05)
    groups = [(g[0], g[1], 2, None) for g in m.groups]
    if name == "mixed1_empty_middle":       # fx_nl_init_groups makes no part of it: fx_nl_nodal_stress concatenates the parts that are left
        groups.insert(1, (groups[2][0], np.zeros((0, groups[2][1].shape[1]), dtype=np.int32), 2, None))
    return m, groups, [mises(fstr.TOTALLAG)]


@pytest.mark.parametrize("name", ["bbar", "fbar", "mixed1", "mixed2", "mixed1_empty_middle"])
def test_resident_state_of_a_nonlinear_context(hip, name):
    """fx_nl_nodal_stress after three Newton sub-steps with a Mises material: byte for byte fx_nodal_stress_groups fed with the
    context's get_state() arrays, equal to the restatement of that state, its summary equal to the existing helpers' to the
    printed digits; and fstr_NodalStress3D fills fstrSOLID."""
    import thermal_ref
    from frontistr_amd import fstr
    m, groups, mats = _nl_case(name)
    c, solid = _newton(hip, m.coord, groups, mats, _stretch(m))
    try:
        s = solid.get_state(("stress", "strain", "plstrain", "unode"))
        assert (s["plstrain"] > 0).any(), "no plastic point"
        res = solid.nodal_stress(principal=ALL)
        again = solid.nodal_stress(principal=ALL)
        held = [k for k, g in enumerate(groups) if g[1].shape[0]]       # the flat arrays hold these, one after the other
        full = [groups[k] for k in held]
        lin = c.nodal_stress_groups(m.n_node, full, s["strain"].ravel(), s["stress"].ravel(), principal=ALL)
        for k in ARRAYS:
            assert getattr(res, k).tobytes() == getattr(lin, k).tobytes() == getattr(again, k).tobytes(), k
        assert c.nodal_stats()["lists_nl"] == 1
        plain = [(g[0], g[1]) for g in full]
        ref = NR.nodal_stress(m.n_node, plain, s["strain"].ravel(), s["stress"].ravel(), principal=ALL)
        compare(res, ref, ALL, "nonlinear " + name)
        strains, stresses = ([a[k] for k in held] for a in (solid.group_slices("strain", s["strain"]), solid.group_slices("stress", s["stress"])))
        want = thermal_ref.summary(plain, s["unode"], strains, stresses)     # c3_nl_ref / tet_nl_ref underneath, and 361
        got = res.summary(s["unode"])
        print(got, want)
        assert got == want
        r = fstr.fstr_NodalStress3D(solid, principal=hip.PRINC_NSTRESS)
        assert np.array_equal(solid.STRESS, res.stress) and np.array_equal(solid.EMISES, res.emises)
        assert np.array_equal(solid.PSTRESS, res.pstress) and solid.PSTRESS_VECT is None and r.pstrain is None
    finally:
        c.close()
