"""Device assembly and linear stress update of tetrahedra (TYPE=341, 342) against the numpy restatement tests/tet_ref.py.

Element matrices (fx_element_stiffness_c3) to 1e-13 relative on distorted elements; assembled matrices (fx_assemble_c3) to
1e-12 of the largest entry with one material, several sections, nonzero Dirichlet values and scrambled numbering, on every
scatter path (coloured with first-write flags, FX_ASM_FIRST=0, FX_ASM_MAP=0, FX_ASM_ATOMIC=1; the switches are read once per
process, so each non-default path runs in a fresh child); two coloured assemblies bit for bit; a hexahedron and a tetrahedron
assembly on one context in both orders (the colour / map cache is keyed by element type); the stress update
(fx_update_c3_linear) to 1e-12 (strain, stress) and 1e-11 (QFORCE, fp64 atomics); CG + SSOR and CG + DIAG solves of a
device-assembled system against the same solve of the restated matrix; a bad element type and a degenerate element are
errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tet_ref as T
from frontistr_amd.mesh import CubeMesh, TetMesh, renumber

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E, NU = 210000.0, 0.3
FX_ERROR_UNSUPPORTED = -2          # include/fistr_hip.h

MESHES = {
    "t341": lambda: TetMesh(3, etype=341, skew=0.1),
    "t342": lambda: TetMesh(2, etype=342, skew=0.1, curve=0.04),
    "t341_renum": lambda: renumber(TetMesh(3, etype=341, skew=0.1), 21),
    "t342_renum": lambda: renumber(TetMesh(2, etype=342, skew=0.1, curve=0.04), 22),
}
ETYPE = {"t341": 341, "t342": 342, "t341_renum": 341, "t342_renum": 342}
PATHS = {
    "default": None,
    "first0": {"FX_ASM_FIRST": "0"},
    "map0": {"FX_ASM_MAP": "0"},
    "atomic": {"FX_ASM_ATOMIC": "1"},
}


def bc_of(m):
    """The z=0 clamp plus nonzero prescribed values on three nodes of the top face."""
    node, dof, val = m.dirichlet()
    top = [int(n) for n in m.top_nodes[:3]]
    tn = np.repeat(np.array(top, dtype=np.int32), 3)
    td = np.tile(np.array([1, 2, 3], dtype=np.int32), 3)
    tv = 1e-3 * np.sin(1.0 + np.arange(tn.size))
    return np.concatenate([node, tn]), np.concatenate([dof, td]), np.concatenate([val, tv])


def sections_of(m):
    return np.array([210000.0, 70000.0, 150000.0]), np.array([0.3, 0.33, 0.25]), (1 + np.arange(m.n_elem) % 3).astype(np.int32)


def profile(hip, m, nn):
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = nn
    hm.elem_node_item = m.conn.ravel()
    return hip.hecmw_mat_con(hm, hip.hecmwST_matrix())


def device_case(hip, name, variant):
    m = MESHES[name]()
    et = ETYPE[name]
    mat = profile(hip, m, T.NN[et])
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    if variant == "sections":
        Es, nus, em = sections_of(m)
        ctx.assemble_c3(m.coord, m.conn, et, Es, nus, load=m.load(), bc=bc_of(m), elem_mat=em)
    else:
        ctx.assemble_c3(m.coord, m.conn, et, E, NU, load=m.load(), bc=bc_of(m))
    ctx.download_matrix(mat)
    ctx.close()
    return mat


CASES = [(n, v) for n in MESHES for v in ("one", "sections")]


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
    tmp = tmp_path_factory.mktemp("tet_paths")
    compute_all(str(tmp / "default.npz"))
    compute_all(str(tmp / "default_again.npz"))
    for path, env in PATHS.items():
        if env is None:
            continue
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_tet_assembly as T; T.compute_all(%r)" % (
            HERE, ROOT, str(tmp / (path + ".npz")))
        try:
            p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            pytest.fail("scatter path %s: child timed out" % path)
        if p.returncode != 0:
            pytest.fail("scatter path %s: child exited with %d\n%s" % (path, p.returncode, p.stdout[-3000:]))
    return {p: dict(np.load(str(tmp / (p + ".npz")))) for p in list(PATHS) + ["default_again"]}


_REF = {}


def reference(name, variant):
    if (name, variant) not in _REF:
        from frontistr_amd import hecmw as hip
        m = MESHES[name]()
        et = ETYPE[name]
        K, f = T.assemble(et, m.coord, m.conn, E, NU, bc=bc_of(m), load=m.load(),
                          sections=sections_of(m) if variant == "sections" else None)
        mat = profile(hip, m, T.NN[et])
        D, AL, AU = T.to_blocks(K, mat)
        _REF[(name, variant)] = {"D": D, "AL": AL, "AU": AU, "B": f, "K": K, "mat": mat}
    return _REF[(name, variant)]


@pytest.mark.parametrize("etype", [341, 342])
def test_element_stiffness_matches_restatement(etype):
    from frontistr_amd import hecmw as hip
    ctx = hip.SolverContext()
    rng = np.random.default_rng(etype)
    for _ in range(4):
        v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) + 0.15 * rng.standard_normal((4, 3))
        ec = v if etype == 341 else np.concatenate(
            [v, np.array([0.5 * (v[a] + v[b]) for a, b in T.TET10_EDGES]) + 0.03 * rng.standard_normal((6, 3))])
        k = ctx.element_stiffness_c3(etype, ec, E, NU)
        ref = T.element_stiffness(etype, ec, E, NU)
        assert np.abs(k - ref).max() <= 1e-13 * np.abs(ref).max()
    ctx.close()


@pytest.mark.parametrize("name,variant", CASES)
def test_assembly_matches_restatement(results, name, variant):
    ref = reference(name, variant)
    key = "%s-%s" % (name, variant)
    scale = np.abs(ref["D"]).max()
    for path in PATHS:
        r = results[path]
        for k in ("D", "AL", "AU"):
            assert np.abs(r[key + "/" + k] - ref[k]).max() <= 1e-12 * scale, (path, k)
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


def test_hexahedra_and_tetrahedra_share_a_context():
    """CubeMesh(n) and TetMesh(n, 341) have the same nodes, and every tetrahedron lies in one hexahedron: one profile serves
    both.  Assembling 361, 341, 361 (and 341, 361, 341) on one context must give each its own matrix.  (These two meshes differ
    in element count and connectivity checksum, so this pins the rebuild of the cached colours and map on a switch of mesh on a
    shared profile; the element-type part of the cache key only matters when count and checksum coincide, which no pair of
    real meshes here produces.)"""
    from frontistr_amd import hecmw as hip
    hexes, tets = CubeMesh(3, skew=0.1), TetMesh(3, etype=341, skew=0.1)
    assert np.array_equal(hexes.coord, tets.coord)
    mat = profile(hip, hexes, 8)
    K, _ = T.assemble(341, tets.coord, tets.conn, E, NU)
    tD, tAL, tAU = T.to_blocks(K, mat)

    def run(ctx, kind):
        if kind == "hex":
            ctx.assemble_c3d8(hexes.coord, hexes.conn, E, NU, elemopt=3)
        else:
            ctx.assemble_c3(tets.coord, tets.conn, 341, E, NU)
        ctx.download_matrix(mat)
        return mat.D.copy(), mat.AL.copy(), mat.AU.copy()

    for order in (("hex", "tet", "hex"), ("tet", "hex", "tet")):
        ctx = hip.SolverContext()
        ctx.upload(mat, what=hip.FX_UP_PROFILE)
        got = [run(ctx, kind) for kind in order]
        ctx.close()
        fresh = hip.SolverContext()
        fresh.upload(mat, what=hip.FX_UP_PROFILE)
        alone = {kind: run(fresh, kind) for kind in ("hex", "tet")}
        fresh.close()
        for kind, g in zip(order, got):
            for x, y in zip(g, alone[kind]):
                assert np.array_equal(x, y), (order, kind)
        scale = np.abs(tD).max()
        t = alone["tet"]
        for x, y in zip(t, (tD, tAL, tAU)):
            assert np.abs(x - y).max() <= 1e-12 * scale
        assert np.abs(alone["hex"][1]).max() > 0 and np.count_nonzero(alone["hex"][1]) > np.count_nonzero(t[1])


@pytest.mark.parametrize("name", list(MESHES))
def test_update_matches_restatement(name):
    from frontistr_amd import hecmw as hip
    m = MESHES[name]()
    et = ETYPE[name]
    rng = np.random.default_rng(7)
    u = 1e-3 * rng.standard_normal(m.ndof)
    Es, nus, em = sections_of(m)
    ctx = hip.SolverContext()
    for sec in (False, True):
        if sec:
            s, st, q, _ = ctx.update_c3_linear(m.coord, m.conn, et, Es, nus, u, elem_mat=em)
            rs, rst, rq = T.update(et, m.coord, m.conn, Es, nus, u, elem_mat=em)
        else:
            s, st, q, _ = ctx.update_c3_linear(m.coord, m.conn, et, E, NU, u)
            rs, rst, rq = T.update(et, m.coord, m.conn, E, NU, u)
        assert s.shape == (m.n_elem, T.nq(et), 6)
        assert np.abs(s - rs).max() <= 1e-12 * np.abs(rs).max()
        assert np.abs(st - rst).max() <= 1e-12 * np.abs(rst).max()
        assert np.abs(q - rq).max() <= 1e-11 * np.abs(rq).max()
    ctx.close()


@pytest.mark.parametrize("etype,precond", [(341, 1), (342, 1), (342, 3)])
def test_solve_of_device_assembled_tets(etype, precond):
    """CG + SSOR (1) / DIAG (3) on the device-assembled system against the CPU oracle's same solve of the restated matrix."""
    from frontistr_amd import hecmw as hip
    from oracle import pyoracle as po
    from oracle.refrun import default_params
    m = TetMesh(3, etype=etype, skew=0.08, curve=0.03 if etype == 342 else 0.0)
    mat = profile(hip, m, T.NN[etype])
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_c3(m.coord, m.conn, etype, E, NU, load=m.load(), bc=m.dirichlet())
    mat.Iarray[0] = 10000
    mat.Iarray[1] = 1
    mat.Iarray[2] = precond
    code = ctx.solve_resident(mat)
    ctx.download_x(mat)
    iters = ctx.info.iterations
    ctx.close()
    K, f = T.assemble(etype, m.coord, m.conn, E, NU, bc=m.dirichlet(), load=m.load())
    D, AL, AU = T.to_blocks(K, mat)
    ref = hip.hecmwST_matrix.from_arrays(mat.N, mat.NP, mat.indexL, mat.itemL, mat.indexU, mat.itemU, D, AL, AU, B=f)
    I, R = default_params(method=1, precond=precond)
    o = po.solve_iterative(ref, I, R, nthreads=1 if precond == 3 else 4)
    assert code == 0
    assert abs(iters - o["iter"]) <= 1, (iters, o["iter"])
    assert np.abs(mat.X - o["X"]).max() <= 1e-8 * np.abs(o["X"]).max()
    x = np.linalg.solve(K, f)
    assert np.abs(mat.X - x).max() <= 1e-6 * np.abs(x).max()


def test_bad_etype_and_degenerate_element_are_errors():
    from frontistr_amd import hecmw as hip
    m = TetMesh(1, etype=341)
    mat = profile(hip, m, 4)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_c3(m.coord, m.conn, 343, E, NU)
    assert e.value.code == FX_ERROR_UNSUPPORTED
    with pytest.raises(hip.HecmwSolverError):
        ctx.update_c3_linear(m.coord, m.conn, 361, E, NU, np.zeros(m.ndof))
    with pytest.raises(hip.HecmwSolverError):
        ctx.element_stiffness_c3(10, np.zeros((4, 3)), E, NU)
    bad = m.conn.copy()
    bad[2, 3] = bad[2, 0]                                  # a tetrahedron naming a node twice
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_c3(m.coord, bad, 341, E, NU)
    assert "twice" in str(e.value)
    with pytest.raises(hip.HecmwSolverError):
        ctx.update_c3_linear(m.coord, bad, 341, E, NU, np.zeros(m.ndof))
    # the context still works afterwards
    ctx.assemble_c3(m.coord, m.conn, 341, E, NU, bc=m.dirichlet())
    ctx.download_matrix(mat)
    K, _ = T.assemble(341, m.coord, m.conn, E, NU, bc=m.dirichlet())
    D, AL, AU = T.to_blocks(K, mat)
    assert np.abs(mat.D - D).max() <= 1e-12 * np.abs(D).max()
    ctx.close()


@pytest.mark.parametrize("deck", T.GOLDEN_DECKS, ids=[d[0] for d in T.GOLDEN_DECKS])
def test_assembly_matches_the_reference_dump(deck):
    """fx_assemble_c3 against the unmodified fistr1's own assembled K after the boundary conditions and its right-hand side
    (tests/golden/tet_decks.npz, printed with 12 digits): 1e-11 of the largest entry."""
    from frontistr_amd import hecmw as hip
    g = np.load(os.path.join(HERE, "golden", "tet_decks.npz"))
    m, sec, Kd, Bd = T.golden_deck(g, *deck)
    mat = profile(hip, m, T.NN[deck[1]])
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    if sec is None:
        ctx.assemble_c3(m.coord, m.conn, deck[1], T.DECK_E[0], T.DECK_NU[0], load=m.load(), bc=m.dirichlet())
    else:
        ctx.assemble_c3(m.coord, m.conn, deck[1], sec[0], sec[1], load=m.load(), bc=m.dirichlet(), elem_mat=sec[2])
    ctx.download_matrix(mat)
    ctx.close()
    assert np.abs(T.dense_of(mat) - Kd).max() <= 1e-11 * np.abs(Kd).max()
    assert np.abs(mat.B - Bd).max() <= 1e-11 * max(np.abs(Bd).max(), 1.0)
