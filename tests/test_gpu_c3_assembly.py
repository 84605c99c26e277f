"""Device assembly and linear stress update of wedges and 20-node hexahedra (TYPE=351, 352, 362) against the numpy restatement
tests/c3_ref.py, which tests/test_c3_ref.py pins to the unmodified reference.

Must fail without the feature: before these element types had kernels, every test here that calls assemble_c3,
update_c3_linear or element_stiffness_c3 with etype 351, 352 or 362 raised FX_ERROR_UNSUPPORTED.

Element matrices (fx_element_stiffness_c3) to 1e-13 of the largest entry on distorted elements (the tetrahedra's bound), symmetric, the six rigid-body
modes at zero energy; assembled matrices (fx_assemble_c3) to 1e-12 of the largest entry (the bound of
test_gpu_tet_assembly.py) on straight and distorted meshes with one material, several sections, nonzero Dirichlet values,
without Dirichlet rows and with scrambled numbering, at sizes that give several colours and more than one workgroup in a
colour, on every scatter path (coloured with first-write flags, FX_ASM_FIRST=0, FX_ASM_MAP=0, FX_ASM_ATOMIC=1; the switches
are read once per process, so each non-default path runs in a fresh child); two coloured assemblies bit for bit; the
reference's own K (tests/golden/c3_decks.npz) to 1e-11; the stress update (fx_update_c3_linear) to 1e-12 (strain, stress) and
1e-11 (QFORCE, fp64 atomics) and the patch test on distorted meshes; CG + SSOR solves of a device-assembled system against the
same solve of the restated matrix and a dense solve; an element naming a node twice is refused for each type and the context
works afterwards; etype 343 stays FX_ERROR_UNSUPPORTED."""
import os
import subprocess
import sys

import numpy as np
import pytest

import c3_ref as T
from frontistr_amd.mesh import C3_POINTS, color_elements, renumber, solid_mesh

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E, NU = 210000.0, 0.3
FX_ERROR_UNSUPPORTED = -2          # include/fistr_hip.h

MESHES = {
    "w351": lambda: solid_mesh(6, 351, skew=0.1),                       # 432 elements, 13 colours, 12 elements per workgroup
    "w352": lambda: solid_mesh(3, 352, skew=0.1, curve=0.04),           # 54 elements, 13 colours, 2 per workgroup
    "h362": lambda: solid_mesh(3, 362, skew=0.1, curve=0.04),           # 27 elements, 8 colours, 1 per workgroup
    "w352_straight": lambda: solid_mesh(2, 352),
    "h362_straight": lambda: solid_mesh(2, 362),
    "w351_renum": lambda: renumber(solid_mesh(4, 351, skew=0.1), 20),
    "w352_renum": lambda: renumber(solid_mesh(2, 352, skew=0.1, curve=0.04), 21),
    "h362_renum": lambda: renumber(solid_mesh(2, 362, skew=0.1, curve=0.04), 22),
}
ETYPE = {k: int(k[1:4]) for k in MESHES}
ELEMS_PER_WORKGROUP = {351: 12, 352: 2, 362: 1}                         # fx_assemble_c3.h
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
    elif variant == "nobc":
        ctx.assemble_c3(m.coord, m.conn, et, E, NU, load=m.load())
    else:
        ctx.assemble_c3(m.coord, m.conn, et, E, NU, load=m.load(), bc=bc_of(m))
    ctx.download_matrix(mat)
    ctx.close()
    return mat


CASES = [(n, v) for n in MESHES for v in ("one", "sections")] + [(n, "nobc") for n in ("w351", "w352", "h362")]


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
    tmp = tmp_path_factory.mktemp("c3_paths")
    compute_all(str(tmp / "default.npz"))
    compute_all(str(tmp / "default_again.npz"))
    for path, env in PATHS.items():
        if env is None:
            continue
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_c3_assembly as M; M.compute_all(%r)" % (
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
        K, f = T.assemble(et, m.coord, m.conn, E, NU, bc=None if variant == "nobc" else bc_of(m), load=m.load(),
                          sections=sections_of(m) if variant == "sections" else None)
        mat = profile(hip, m, T.NN[et])
        D, AL, AU = T.to_blocks(K, mat)
        _REF[(name, variant)] = {"D": D, "AL": AL, "AU": AU, "B": f, "K": K, "mat": mat}
    return _REF[(name, variant)]


def test_the_meshes_give_several_colours_and_workgroups():
    """What the sizes above are chosen for: several colours, and a colour that needs more than one workgroup."""
    for name in ("w351", "w352", "h362"):
        m = MESHES[name]()
        col = color_elements(m.conn, m.n_node)
        assert col is not None and col.max() + 1 >= 4
        assert np.bincount(col).max() > ELEMS_PER_WORKGROUP[ETYPE[name]], name


@pytest.mark.parametrize("etype", [351, 352, 362])
def test_element_stiffness_matches_restatement(etype):
    from frontistr_amd import hecmw as hip
    ctx = hip.SolverContext()
    rng = np.random.default_rng(etype)
    for _ in range(4):
        A = np.eye(3) + 0.15 * rng.standard_normal((3, 3))
        ec = T.natural_nodes(etype) @ A.T
        ec = ec + 0.03 * rng.standard_normal(ec.shape)
        assert (T.element_dets(etype, ec) > 0).all()
        k = ctx.element_stiffness_c3(etype, ec, E, NU)
        ref = T.element_stiffness(etype, ec, E, NU)
        scale = np.abs(ref).max()
        print("etype %d: |k - ref| / max|ref| = %.3e" % (etype, np.abs(k - ref).max() / scale))
        assert np.abs(k - ref).max() <= 1e-13 * scale
        assert np.abs(k - k.T).max() <= 1e-14 * scale       # (a diagonal block is one lane's sum: symmetric to rounding)
        rb = np.zeros((3 * ec.shape[0], 6))                # three translations, three small rotations
        for d in range(3):
            rb[d::3, d] = 1.0
        for q, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
            rb[i::3, 3 + q] = -ec[:, j]
            rb[j::3, 3 + q] = ec[:, i]
        assert np.abs(k @ rb).max() <= 1e-11 * scale
        ev = np.linalg.eigvalsh(k) / scale
        assert (np.abs(ev[:6]) < 1e-12).all()
        if etype != 351:   # (351's two-point rule leaves the reference's element further zero-energy modes: test_c3_ref.py)
            assert ev[6] > 1e-7
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
        assert s.shape == (m.n_elem, C3_POINTS[et], 6)
        assert np.abs(s - rs).max() <= 1e-12 * np.abs(rs).max()
        assert np.abs(st - rst).max() <= 1e-12 * np.abs(rst).max()
        assert np.abs(q - rq).max() <= 1e-11 * np.abs(rq).max()
    ctx.close()


@pytest.mark.parametrize("etype,precond", [(351, 1), (352, 1), (362, 1)])
def test_solve_of_device_assembled_elements(etype, precond):
    """CG + SSOR (1) / DIAG (3) on the device-assembled system against the CPU oracle's same solve of the restated matrix."""
    from frontistr_amd import hecmw as hip
    from oracle import pyoracle as po
    from oracle.refrun import default_params
    m = solid_mesh(3, etype, skew=0.08, **({} if etype == 351 else {"curve": 0.03}))
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


@pytest.mark.parametrize("etype", [352, 362])
def test_patch_linear_field_on_the_device(etype):
    """u = A x + c on a distorted mesh: the constant strain sym(A) and its stress at every quadrature point."""
    from frontistr_amd import hecmw as hip
    m = solid_mesh(3, etype, skew=0.1, curve=0.04)
    A = 1e-3 * np.random.default_rng(3).standard_normal((3, 3))
    u = (m.coord @ A.T + 1e-3).ravel()
    ctx = hip.SolverContext()
    strain, stress, _, _ = ctx.update_c3_linear(m.coord, m.conn, etype, E, NU, u)
    ctx.close()
    eps = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1] + A[1, 0], A[1, 2] + A[2, 1], A[2, 0] + A[0, 2]])
    assert strain.shape == (m.n_elem, C3_POINTS[etype], 6)
    assert np.abs(strain - eps).max() <= 1e-12 * np.abs(eps).max()           # the bounds of test_c3_ref.py's patch test
    assert np.abs(stress - T.elastic_matrix(E, NU) @ eps).max() <= 1e-9 * np.abs(stress).max()


@pytest.mark.parametrize("etype", [351, 352, 362])
def test_bad_etype_and_degenerate_element_are_errors(etype):
    from frontistr_amd import hecmw as hip
    m = solid_mesh(1, etype)
    nn = T.NN[etype]
    mat = profile(hip, m, nn)
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_c3(m.coord, m.conn, 343, E, NU)
    assert e.value.code == FX_ERROR_UNSUPPORTED
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.update_c3_linear(m.coord, m.conn, 343, E, NU, np.zeros(m.ndof))
    assert e.value.code == FX_ERROR_UNSUPPORTED
    bad = m.conn.copy()
    bad[0, nn - 1] = bad[0, 0]                             # an element naming a node twice
    with pytest.raises(hip.HecmwSolverError) as e:
        ctx.assemble_c3(m.coord, bad, etype, E, NU)
    assert "twice" in str(e.value)
    with pytest.raises(hip.HecmwSolverError):
        ctx.update_c3_linear(m.coord, bad, etype, E, NU, np.zeros(m.ndof))
    # the context still works afterwards
    ctx.assemble_c3(m.coord, m.conn, etype, E, NU, bc=m.dirichlet())
    ctx.download_matrix(mat)
    K, _ = T.assemble(etype, m.coord, m.conn, E, NU, bc=m.dirichlet())
    D, AL, AU = T.to_blocks(K, mat)
    assert np.abs(mat.D - D).max() <= 1e-12 * np.abs(D).max()
    ctx.close()


@pytest.mark.parametrize("deck", T.GOLDEN_DECKS, ids=[d[0] for d in T.GOLDEN_DECKS])
def test_assembly_matches_the_reference_dump(deck):
    """fx_assemble_c3 against the unmodified fistr1's own assembled K after the boundary conditions and its right-hand side
    (tests/golden/c3_decks.npz, printed with 12 digits): 1e-11 of the largest entry."""
    from frontistr_amd import hecmw as hip
    g = np.load(os.path.join(HERE, "golden", "c3_decks.npz"))
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
