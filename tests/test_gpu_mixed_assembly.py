"""Device assembly and linear stress update of a mesh of SEVERAL solid element types (fx_assemble_groups,
fx_update_groups_linear) against the restatement tests/mixed_ref.py, which tests/test_mixed_ref.py pins to the unmodified
reference.

Must fail without the feature: libfistr_hip.so had no fx_assemble_groups / fx_update_groups_linear symbol.

Assembled matrices to 1e-12 of the largest entry (the bound of test_gpu_c3_assembly.py) on MixedMesh order 1 and 2, n in {2, 5},
skewed, one and several materials, with and without boundary conditions and load, after renumbering, on every scatter path
(coloured with the first-write flags of the global launch order, FX_ASM_FIRST=0, FX_ASM_MAP=0, FX_ASM_ATOMIC=1 -- the switches
are read once per process, so each non-default path runs in a fresh child; the paths agree to 1e-13 as in the single-type
tests); the group order permuted; two assemblies bit for bit, also after another mesh was assembled in between (the per-group
colour / map cache); one group through assemble_groups bit for bit the single-type entry point, for each of the six types; a
collapsed 361 element inside a mixed mesh; a degenerate wedge and an unknown type refused with the matrix of the previous
assembly untouched; the single-type entry points run the same group driver: their calls and multi-group calls alternate on one
context (one cache) bit for bit, they refuse a bad node id before anything is uploaded, and the pinned staging of the stress
update belongs to its context; the stress update to 1e-11; CG + SSOR and CG + ILU(0) solves of the device-assembled mixed system against
the dense solve of the restated one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_ref as M
from frontistr_amd.mesh import C3_POINTS, CubeMesh, MixedMesh, renumber_groups, solid_mesh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E, NU = 210000.0, 0.3
FX_ERROR_RUNTIME, FX_ERROR_UNSUPPORTED = -1, -2          # include/fistr_hip.h

MESHES = {
    "m1_n2": lambda: MixedMesh(2, order=1, skew=0.1),
    "m1_n5": lambda: MixedMesh(5, order=1, skew=0.1),                     # 20 + 120 + 270 elements
    "m2_n2": lambda: MixedMesh(2, order=2, skew=0.1, curve=0.04),
    "m2_n5": lambda: MixedMesh(5, order=2, skew=0.08, curve=0.03),
    "m1_n5_renum": lambda: renumber_groups(MixedMesh(5, order=1, skew=0.1), 31),
    "m2_n2_renum": lambda: renumber_groups(MixedMesh(2, order=2, skew=0.1, curve=0.04), 32),
}
PATHS = {"default": None, "first0": {"FX_ASM_FIRST": "0"}, "map0": {"FX_ASM_MAP": "0"}, "atomic": {"FX_ASM_ATOMIC": "1"}}
SEC_E, SEC_NU = np.array([210000.0, 70000.0, 150000.0]), np.array([0.3, 0.33, 0.25])


def bc_of(m):
    """The z=0 clamp plus nonzero prescribed values on three nodes of the top face."""
    node, dof, val = m.dirichlet()
    tn = np.repeat(np.array([int(n) for n in m.top_nodes[:3]], dtype=np.int32), 3)
    td = np.tile(np.array([1, 2, 3], dtype=np.int32), 3)
    tv = 1e-3 * np.sin(1.0 + np.arange(tn.size))
    return np.concatenate([node, tn]), np.concatenate([dof, td]), np.concatenate([val, tv])


def groups_of(m, variant):
    if variant == "sections":
        return m.groups_with(elemopt=2, elem_mat=(1 + np.arange(m.n_elem) % 3).astype(np.int32)), SEC_E, SEC_NU
    return m.groups, E, NU


def inputs(name, variant):
    m = MESHES[name]()
    groups, Es, nus = groups_of(m, variant)
    if variant == "tets_first":
        groups = groups[::-1]
    return m, groups, Es, nus, (None if variant == "nobc" else bc_of(m)), (None if variant == "nobc" else m.load())


def device_case(hip, name, variant):
    m, groups, Es, nus, bc, load = inputs(name, variant)
    mat = M.profile(hip, m.n_node, groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_groups(m.coord, groups, Es, nus, load=load, bc=bc)
    ctx.download_matrix(mat)
    ctx.close()
    return mat


CASES = [(n, v) for n in MESHES for v in ("one", "sections")] + [(n, v) for n in ("m1_n5", "m2_n2") for v in ("nobc", "tets_first")]


def compute_all(path):
    from frontistr_amd import hecmw as hip
    out = {}
    for name, variant in CASES:
        mat = device_case(hip, name, variant)
        for k in ("D", "AL", "AU", "B"):
            out["%s-%s/%s" % (name, variant, k)] = np.array(getattr(mat, k))
    np.savez(path, **out)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mixed_paths")
    compute_all(str(tmp / "default.npz"))
    compute_all(str(tmp / "default_again.npz"))
    for path, env in PATHS.items():
        if env is None:
            continue
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_mixed_assembly as T; T.compute_all(%r)" % (
            HERE, ROOT, str(tmp / (path + ".npz")))
        try:
            p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            pytest.fail("scatter path %s: child timed out" % path)
        if p.returncode != 0:
            pytest.fail("scatter path %s: child exited with %d\n%s" % (path, p.returncode, p.stdout[-3000:]))
    return {p: dict(np.load(str(tmp / (p + ".npz")))) for p in list(PATHS) + ["default_again"]}


_REF = {}


def reference(name, variant):
    if (name, variant) not in _REF:
        from frontistr_amd import hecmw as hip
        m, groups, Es, nus, bc, load = inputs(name, variant)
        K, f = M.assemble(m.coord, groups, Es, nus, bc=bc, load=load)
        D, AL, AU = M.to_blocks(K, M.profile(hip, m.n_node, groups))
        _REF[(name, variant)] = {"D": D, "AL": AL, "AU": AU, "B": f}
    return _REF[(name, variant)]


@pytest.mark.parametrize("name,variant", CASES)
def test_assembly_matches_restatement_on_every_scatter_path(results, name, variant):
    ref = reference(name, variant)
    key = "%s-%s" % (name, variant)
    scale = np.abs(ref["D"]).max()
    for path in PATHS:
        r = results[path]
        for k in ("D", "AL", "AU"):
            err = np.abs(r[key + "/" + k] - ref[k]).max() / scale
            print("%s %s %s: %.3e" % (key, path, k, err))
            assert err <= 1e-12, (path, k)
        assert np.abs(r[key + "/B"] - ref["B"]).max() <= 1e-12 * max(np.abs(ref["B"]).max(), 1.0), path


@pytest.mark.parametrize("name,variant", CASES)
def test_scatter_paths_agree_and_coloured_is_reproducible(results, name, variant):
    key = "%s-%s" % (name, variant)
    d = results["default"]
    for k in ("D", "AL", "AU", "B"):
        assert np.array_equal(d[key + "/" + k], results["default_again"][key + "/" + k]), k
        scale = max(np.abs(d[key + "/" + k]).max(), 1.0)
        for path in ("first0", "map0", "atomic"):
            assert np.abs(results[path][key + "/" + k] - d[key + "/" + k]).max() <= 1e-13 * scale, (path, k)


@pytest.mark.parametrize("name", ["m1_n5", "m2_n2"])
def test_group_order_permuted_gives_the_same_matrix(results, name):
    a, b = "%s-one" % name, "%s-tets_first" % name
    scale = np.abs(results["default"][a + "/D"]).max()
    for k in ("D", "AL", "AU", "B"):
        assert np.abs(results["default"][a + "/" + k] - results["default"][b + "/" + k]).max() <= 1e-12 * scale, k


def _arrays(ctx, mat):
    ctx.download_matrix(mat)
    return {k: np.array(getattr(mat, k)) for k in ("D", "AL", "AU", "B")}


def test_second_assembly_reuses_the_cache_bit_for_bit():
    """The same groups again, and again after another mesh (other groups, then a single-type call) went through the context."""
    from frontistr_amd import hecmw as hip
    m = MESHES["m1_n5"]()
    groups = m.groups
    mat = M.profile(hip, m.n_node, groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_groups(m.coord, groups, E, NU, load=m.load(), bc=bc_of(m))
    first = _arrays(ctx, mat)
    ctx.assemble_groups(m.coord, groups, E, NU, load=m.load(), bc=bc_of(m))
    second = _arrays(ctx, mat)
    other = [(groups[0][0], groups[0][1], 3, None), (groups[2][0], groups[2][1], 1, None), (groups[1][0], groups[1][1], 1, None)]
    ctx.assemble_groups(m.coord, other, E, NU)                             # the same profile, other groups in the cache slots
    ctx.assemble_groups(m.coord, [groups[1]], E, NU)                       # and the single-type path
    ctx.assemble_groups(m.coord, groups, E, NU, load=m.load(), bc=bc_of(m))
    third = _arrays(ctx, mat)
    ctx.close()
    for k in first:
        assert np.array_equal(first[k], second[k]) and np.array_equal(first[k], third[k]), k


ONE_GROUP = {361: lambda: CubeMesh(4, skew=0.1), 341: lambda: solid_mesh(3, 341, skew=0.1),
             342: lambda: solid_mesh(2, 342, skew=0.1, curve=0.04), 351: lambda: solid_mesh(3, 351, skew=0.1),
             352: lambda: solid_mesh(2, 352, skew=0.1, curve=0.04), 362: lambda: solid_mesh(2, 362, skew=0.1, curve=0.04)}


@pytest.mark.parametrize("etype", sorted(ONE_GROUP))
@pytest.mark.parametrize("sections", [False, True])
def test_one_group_equals_the_single_type_entry_point_bitwise(etype, sections):
    from frontistr_amd import hecmw as hip
    m = ONE_GROUP[etype]()
    em = (1 + np.arange(m.n_elem) % 3).astype(np.int32) if sections else None
    Es, nus = (SEC_E, SEC_NU) if sections else (E, NU)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    out = []
    for grouped in (False, True):
        mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        ctx = hip.SolverContext()
        ctx.upload(mat, what=hip.FX_UP_PROFILE)
        if grouped:
            ctx.assemble_groups(m.coord, [(etype, m.conn, 2, em)], Es, nus, load=m.load(), bc=bc_of(m))
        elif etype == 361:
            ctx.assemble_c3d8(m.coord, m.conn, E, NU, elemopt=2, load=m.load(), bc=bc_of(m), sections=(Es, nus, em) if sections else None)
        else:
            ctx.assemble_c3(m.coord, m.conn, etype, Es, nus, load=m.load(), bc=bc_of(m), elem_mat=em)
        out.append(_arrays(ctx, mat))
        u = 1e-3 * np.random.default_rng(etype).standard_normal(m.ndof)
        if grouped:
            s, t, q, _ = ctx.update_groups_linear(m.coord, [(etype, m.conn, 2, em)], Es, nus, u)
            out[-1].update(strain=s[0], stress=t[0], q=q)
        elif etype == 361:
            s, t, q, _ = ctx.update_c3d8_linear(m.coord, m.conn, Es, nus, u, elemopt=2, elem_mat=em)
            out[-1].update(strain=s, stress=t, q=q)
        else:
            s, t, q, _ = ctx.update_c3_linear(m.coord, m.conn, etype, Es, nus, u, elem_mat=em)
            out[-1].update(strain=s, stress=t, q=q)
        ctx.close()
    for k in ("D", "AL", "AU", "B", "strain", "stress"):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.abs(out[0]["q"] - out[1]["q"]).max() <= 1e-11 * np.abs(out[0]["q"]).max()       # QFORCE: fp64 atomics


def test_collapsed_hexahedron_inside_a_mixed_mesh():
    from frontistr_amd import hecmw as hip
    m = MixedMesh(4, order=1, skew=0.05)
    conns = [c.copy() for c in m.conns]
    conns[0][3, 3] = conns[0][3, 0]                        # nodes 1 and 4 (and 5 and 8) of one hexahedron coincide: a wedge
    conns[0][3, 7] = conns[0][3, 4]
    groups = [(et, c, 3, None) for et, c in zip(m.etypes, conns)]   # FI: the restated STF_C3 takes any 8 node ids
    mat = M.profile(hip, m.n_node, groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_groups(m.coord, groups, E, NU, load=m.load(), bc=m.dirichlet())
    ctx.download_matrix(mat)
    ctx.close()
    K, f = M.assemble(m.coord, groups, E, NU, bc=m.dirichlet(), load=m.load())
    D, AL, AU = M.to_blocks(K, mat)
    scale = np.abs(D).max()
    assert np.abs(mat.D - D).max() <= 1e-12 * scale
    assert np.abs(mat.AL - AL).max() <= 1e-12 * scale and np.abs(mat.AU - AU).max() <= 1e-12 * scale
    assert np.abs(mat.B - f).max() <= 1e-12 * max(np.abs(f).max(), 1.0)


def test_refusals_leave_the_previous_matrix_untouched():
    from frontistr_amd import hecmw as hip
    m = MixedMesh(3, order=1, skew=0.1)
    mat = M.profile(hip, m.n_node, m.groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_groups(m.coord, m.groups, E, NU, load=m.load(), bc=m.dirichlet())
    before = _arrays(ctx, mat)
    bad = [c.copy() for c in m.conns]
    bad[1][4, 5] = bad[1][4, 0]                            # a degenerate wedge: element 5 of group 2
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_groups(m.coord, [(et, c, 1, None) for et, c in zip(m.etypes, bad)], E, NU)
    assert e.value.code == FX_ERROR_RUNTIME and "group 2" in str(e.value) and "element 5" in str(e.value) and "twice" in str(e.value)
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_groups(m.coord, m.groups[:2] + [(343, m.conns[2], 1, None)], E, NU)
    assert e.value.code == FX_ERROR_UNSUPPORTED
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.update_groups_linear(m.coord, m.groups[:2] + [(371, m.conns[2], 1, None)], E, NU, np.zeros(m.ndof))
    assert e.value.code == FX_ERROR_UNSUPPORTED
    for kw in ({"groups": []}, {"E": np.zeros(0), "nu": np.zeros(0)}):
        args = {"groups": m.groups, "E": E, "nu": NU}
        args.update(kw)
        with pytest.raises(hip.HecmwSolverError) as e:
            ctx.assemble_groups(m.coord, args["groups"], args["E"], args["nu"])
        assert e.value.code == FX_ERROR_RUNTIME
    with pytest.raises(hip.HecmwSolverError) as e:         # material id out of range
        ctx.assemble_groups(m.coord, m.groups_with(elem_mat=np.full(m.n_elem, 3, dtype=np.int32)), SEC_E[:2], SEC_NU[:2])
    assert e.value.code == FX_ERROR_RUNTIME and "material" in str(e.value)
    oob = [c.copy() for c in m.conns]
    oob[2][0, 0] = m.n_node + 1
    with pytest.raises(hip.HecmwSolverError) as e:         # node id out of range
        ctx.assemble_groups(m.coord, [(et, c, 1, None) for et, c in zip(m.etypes, oob)], E, NU)
    assert e.value.code == FX_ERROR_RUNTIME and "node id" in str(e.value)
    after = _arrays(ctx, mat)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    ctx.assemble_groups(m.coord, m.groups, E, NU, load=m.load(), bc=m.dirichlet())     # the context still works
    again = _arrays(ctx, mat)
    ctx.close()
    for k in before:
        assert np.array_equal(before[k], again[k]), k


def _fresh(hip, m, groups, call):
    """D / AL / AU / B of call(ctx) on a new context holding the profile of `groups`."""
    mat = M.profile(hip, m.n_node, groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    call(ctx)
    out = _arrays(ctx, mat)
    ctx.close()
    return out


@pytest.mark.parametrize("collapsed", [False, True])
def test_single_type_and_group_calls_share_one_cache_without_stale_flags(collapsed):
    """assemble_c3d8 with the hexahedra alone, assemble_groups with all three groups, the hexahedra alone again, all on the
    profile of the mixed mesh: every call re-colours and re-maps the one cache, and none inherits the other's first-write flags
    (the hexahedra alone do not cover the profile: cleared; the three groups do: first-write, unless a hexahedron is collapsed)."""
    from frontistr_amd import hecmw as hip
    m = MESHES["m1_n2"]()
    conns = [c.copy() for c in m.conns]
    eo = 1
    if collapsed:
        conns[0][1, 3], conns[0][1, 7] = conns[0][1, 0], conns[0][1, 4]
        eo = 3
    groups = [(et, c, eo, None) for et, c in zip(m.etypes, conns)]
    assert groups[0][0] == 361
    load, bc = m.load(), bc_of(m)
    hexes = lambda ctx: ctx.assemble_c3d8(m.coord, conns[0], E, NU, elemopt=eo, load=load, bc=bc)
    mixed = lambda ctx: ctx.assemble_groups(m.coord, groups, E, NU, load=load, bc=bc)
    mat = M.profile(hip, m.n_node, groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    got = []
    for call in (hexes, mixed, hexes):
        call(ctx)
        got.append(_arrays(ctx, mat))
    ctx.close()
    want_hexes, want_mixed = _fresh(hip, m, groups, hexes), _fresh(hip, m, groups, mixed)
    for k in ("D", "AL", "AU", "B"):
        assert np.array_equal(got[0][k], got[2][k]), k
        assert np.array_equal(got[0][k], want_hexes[k]), k
        assert np.array_equal(got[1][k], want_mixed[k]), k
    assert not np.array_equal(got[0]["D"], got[1]["D"])


def test_single_type_entries_refuse_a_bad_node_id_before_anything_is_uploaded():
    from frontistr_amd import hecmw as hip
    m = CubeMesh(3, skew=0.1)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_c3d8(m.coord, m.conn, E, NU, elemopt=1, load=m.load(), bc=m.dirichlet())
    before = _arrays(ctx, mat)
    oob = m.conn.copy()
    oob[5, 2] = m.n_node + 1
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_c3d8(m.coord, oob, E, NU, elemopt=1)
    assert e.value.code == FX_ERROR_RUNTIME and "node id" in str(e.value) and "fx_assemble_c3d8:" in str(e.value)
    after = _arrays(ctx, mat)
    for k in ("D", "AL", "AU", "B"):
        assert np.array_equal(before[k], after[k]), k
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.update_c3d8_linear(m.coord, oob, E, NU, np.zeros(m.ndof), elemopt=1)
    assert e.value.code == FX_ERROR_RUNTIME and "node id" in str(e.value) and "fx_update_c3d8_linear:" in str(e.value)
    ctx.close()


def _update_c3d8_raw(hip, ctx, coord, conn, u):
    """fx_update_c3d8_linear (IC) itself: the library's pointers into the context's pinned staging, not copies."""
    mv = hip._MeshView(coord.shape[0], conn.shape[0], hip._ptr(coord), hip._ptr(conn))
    Es, nus = np.array([E]), np.array([NU])
    ps, pt = C.POINTER(C.c_double)(), C.POINTER(C.c_double)()
    hip._chk(hip.lib().fx_update_c3d8_linear(ctx.h, C.byref(mv), 1, hip._ptr(Es), hip._ptr(nus), None, 1, hip._ptr(u), C.byref(ps),
                                             C.byref(pt), None, None))
    n = 48 * conn.shape[0]
    return np.ctypeslib.as_array(ps, shape=(n,)), np.ctypeslib.as_array(pt, shape=(n,))


def test_update_staging_belongs_to_its_context():
    """Context B pins a larger staging (prepare + update) after context A's update: A's pointers still read A's values, B's
    read B's; after B is destroyed A updates again into the same values."""
    from frontistr_amd import hecmw as hip
    small, big = CubeMesh(2, skew=0.1), CubeMesh(3, skew=0.1)
    coord_a, conn_a = np.ascontiguousarray(small.coord), np.ascontiguousarray(small.conn[:2], dtype=np.int32)   # two elements
    coord_b, conn_b = np.ascontiguousarray(big.coord), np.ascontiguousarray(big.conn, dtype=np.int32)
    ua = 1e-3 * np.random.default_rng(3).standard_normal(3 * small.n_node)
    ub = 1e-3 * np.random.default_rng(4).standard_normal(3 * big.n_node)
    ref = hip.SolverContext()
    want_b = ref.update_c3d8_linear(coord_b, conn_b, E, NU, ub, elemopt=1)[:2]
    ref.close()
    a, b = hip.SolverContext(), hip.SolverContext()
    sa, ta = _update_c3d8_raw(hip, a, coord_a, conn_a, ua)
    keep_s, keep_t = sa.copy(), ta.copy()
    assert np.abs(keep_s).max() > 0 and np.abs(keep_t).max() > 0
    hip._chk(hip.lib().fx_update_c3d8_linear_prepare(b.h, int(conn_b.shape[0])))
    sb, tb = _update_c3d8_raw(hip, b, coord_b, conn_b, ub)
    assert sa.ctypes.data != sb.ctypes.data and ta.ctypes.data != tb.ctypes.data
    assert np.array_equal(sa, keep_s) and np.array_equal(ta, keep_t)
    assert np.array_equal(sb, want_b[0].ravel()) and np.array_equal(tb, want_b[1].ravel())
    del sb, tb
    b.close()
    assert np.array_equal(sa, keep_s) and np.array_equal(ta, keep_t)
    sa2, ta2 = _update_c3d8_raw(hip, a, coord_a, conn_a, ua)
    assert np.array_equal(sa2, keep_s) and np.array_equal(ta2, keep_t)
    del sa, ta, sa2, ta2
    a.close()


@pytest.mark.parametrize("name", ["m1_n5", "m2_n2", "m2_n2_renum"])
def test_update_matches_restatement(name):
    from frontistr_amd import hecmw as hip
    m = MESHES[name]()
    u = 1e-3 * np.random.default_rng(7).standard_normal(3 * m.n_node)
    ctx = hip.SolverContext()
    for variant in ("one", "sections"):
        groups, Es, nus = groups_of(m, variant)
        s, st, q, _ = ctx.update_groups_linear(m.coord, groups, Es, nus, u)
        rs, rst, rq = M.update(m.coord, groups, Es, nus, u)
        for g, (et, conn, _, _) in enumerate(groups):
            assert s[g].shape == (conn.shape[0], 8 if et == 361 else C3_POINTS[et], 6)
            assert np.abs(s[g] - rs[g]).max() <= 1e-11 * np.abs(rs[g]).max(), (variant, et)
            assert np.abs(st[g] - rst[g]).max() <= 1e-11 * np.abs(rst[g]).max(), (variant, et)
        assert np.abs(q - rq).max() <= 1e-11 * np.abs(rq).max()
    ctx.close()


@pytest.mark.parametrize("order,precond", [(1, 1), (1, 10), (2, 1), (2, 10)])
def test_solve_of_the_device_assembled_mixed_system(order, precond):
    """CG + SSOR (1) / ILU(0) (10) on the device-assembled system against the dense solve of the restated one."""
    from frontistr_amd import hecmw as hip
    m = MixedMesh(4 if order == 1 else 3, order=order, skew=0.08, curve=0.03 if order == 2 else 0.0)
    mat = M.profile(hip, m.n_node, m.groups)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_groups(m.coord, m.groups, E, NU, load=m.load(), bc=m.dirichlet())
    mat.Iarray[0] = 10000
    mat.Iarray[1] = 1
    mat.Iarray[2] = precond
    code = ctx.solve_resident(mat)
    ctx.download_x(mat)
    ctx.close()
    K, f = M.assemble(m.coord, m.groups, E, NU, bc=m.dirichlet(), load=m.load())
    x = np.linalg.solve(K, f)
    assert code == 0
    assert np.abs(mat.X - x).max() <= 1e-6 * np.abs(x).max()
