"""Device assembly on irregular meshes against the oracle, on every scatter path.

The meshes (frontistr_amd/mesh.py) are what the structured cubes and golden decks are not: pies whose innermost ring of
hexahedra is collapsed onto the axis (elements that name a node twice), a pie needing exactly 64 element colours, one whose
colouring fails (the atomic fallback), element counts that leave the last workgroup partly filled, a single collapsed
element, randomly renumbered meshes and a hub row wider than FX_BELL_MAXROW.  The scatter switches FX_ASM_FIRST, FX_ASM_MAP
and FX_ASM_ATOMIC are read once per process, so each non-default path runs in a fresh child process that writes its
matrices to an .npz; the parent compares them with the oracle and, where the coloured path runs, bit for bit with the
default path.  Bounds: those of test_assembly_vs_reference_golden (matrix 1e-12 max|D|, B 1e-12 max(|B|, 1)) and of
test_gpu_nonlinear.py (tangent and internal force 1e-11 relative)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frontistr_amd.mesh import CubeMesh, PieMesh, color_elements, renumber

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E, NU = 210000.0, 0.3


class Deck:
    """A golden deck's mesh with the builder interface of frontistr_amd.mesh (for renumber)."""

    def __init__(self, name):
        g = np.load(os.path.join(HERE, "golden", name + ".npz"))
        self.coord, self.conn = g["coord"], g["conn"].astype(np.int32)
        self.n_node, self.n_elem = self.coord.shape[0], self.conn.shape[0]
        self._bc = (g["bc_node"].astype(np.int32), g["bc_dof"].astype(np.int32), g["bc_val"] * 0.01)
        z = self.coord[:, 2]
        self.bottom_nodes = (1 + np.flatnonzero(z <= z.min() + 1e-9)).astype(np.int32)
        self.top_nodes = (1 + np.flatnonzero(z >= z.max() - 1e-9)).astype(np.int32)

    def dirichlet(self):
        return self._bc

    def load(self):
        b = np.zeros(3 * self.n_node)
        b[3 * (self.top_nodes - 1)] = 1.0
        return b


MESHES = {
    "pie24x2x2": lambda: PieMesh(24, 2, 2),             # 48 colours, half the elements collapsed
    "pie32x1x2": lambda: PieMesh(32, 1, 2),             # exactly 64 colours
    "pie33x1x2": lambda: PieMesh(33, 1, 2),             # colouring fails: atomics + binary search
    "pie8x1x1": lambda: PieMesh(8, 1, 1),               # one element per colour
    "pie7x3x1": lambda: PieMesh(7, 3, 1),               # 21 elements: partly filled workgroups
    "wedge1": lambda: PieMesh(8, 1, 1, sectors=1),      # a single collapsed element
    "pie72x2x3": lambda: PieMesh(72, 2, 3),             # hub rows of 219 blocks; colouring fails
    "cube9_renum": lambda: renumber(CubeMesh(9, skew=0.1), 11),
    "pie24x2x2_renum": lambda: renumber(PieMesh(24, 2, 2), 12),
    "necking_renum": lambda: renumber(Deck("nl_necking"), 13),
}
NL_MESHES = ["pie24x2x2", "pie32x1x2", "pie33x1x2", "pie7x3x1", "wedge1", "cube9_renum"]
NL_MATS = ["elastic_ul", "mises_multilinear_ul"]
PATHS = {                                                # scatter path -> environment of its child (None: this process)
    "default": None,
    "first0": {"FX_ASM_FIRST": "0"},
    "map0": {"FX_ASM_MAP": "0"},
    "atomic": {"FX_ASM_ATOMIC": "1"},
    "atomic_map0": {"FX_ASM_ATOMIC": "1", "FX_ASM_MAP": "0"},
}
COLOURED_PATHS = ("default", "first0", "map0")


def mesh(name):
    return MESHES[name]()


def coloured(name):
    m = mesh(name)
    return color_elements(m.conn, m.n_node) is not None


def bc_of(m):
    """The mesh's own clamp plus non-zero prescribed values on three more nodes of the top face: the axis node (if the mesh has
    one) in x only, so that its other rows -- where the collapsed elements' blocks land -- stay in the system, then two others."""
    node, dof, val = m.dirichlet()
    fixed = set(node.tolist())
    top = [int(n) for n in dict.fromkeys(list(getattr(m, "axis_nodes", [])[-1:]) + list(m.top_nodes)) if n not in fixed][:3]
    dofs = [[1] if hasattr(m, "axis_nodes") and k == 0 else [1, 2, 3] for k in range(len(top))]
    tn = np.array([n for n, d in zip(top, dofs) for _ in d], dtype=np.int32)
    td = np.array([x for d in dofs for x in d], dtype=np.int32)
    tv = 1e-3 * np.sin(1.0 + np.arange(tn.size))
    return np.concatenate([node, tn]), np.concatenate([dof, td]), np.concatenate([val, tv])


def linear_cases():
    """(key, mesh name, elemopt, variant) of every linear assembly compared."""
    out = [("%s-eo%d" % (n, eo), n, eo, None) for n in MESHES for eo in (1, 2, 3)]
    out += [("pie24x2x2-sections-eo%d" % eo, "pie24x2x2", eo, "sections") for eo in (1, 2, 3)]
    out += [("pie24x2x2-subset-eo%d" % eo, "pie24x2x2", eo, "subset") for eo in (1, 2, 3)]
    return out


def sections_of(m):
    """Three sections: material id by element index."""
    return np.array([210000.0, 70000.0, 150000.0]), np.array([0.3, 0.33, 0.25]), (1 + np.arange(m.n_elem) % 3).astype(np.int32)


def subset_of(m):
    """The bottom layer's elements on the profile of the whole mesh (rows and blocks no element of the subset touches)."""
    return m.conn[: m.n_elem // m.n_z]


def device_linear(hip, name, eo, variant):
    m = mesh(name)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    conn = subset_of(m) if variant == "subset" else m.conn
    sec = sections_of(m) if variant == "sections" else None
    ctx.assemble_c3d8(m.coord, conn, E, NU, elemopt=eo, load=m.load(), bc=bc_of(m), sections=sec)
    ctx.download_matrix(mat)
    ctx.close()
    return mat


def nl_state(m, plastic):
    from oracle import pyoracle
    rng = np.random.default_rng(m.n_elem)
    st = pyoracle.new_state(m.n_elem)
    st["stress"] = 40.0 * rng.standard_normal((m.n_elem, 8, 6))
    st["stress_bak"] = st["stress"].copy()
    st["strain_bak"] = 1e-4 * rng.standard_normal((m.n_elem, 8, 6))
    st["strain"] = st["strain_bak"].copy()
    if plastic:
        st["plstrain"] = np.abs(1e-3 * rng.standard_normal((m.n_elem, 8)))
        st["fstat"] = st["plstrain"].copy()
    return st, 1e-3 * rng.standard_normal(m.ndof), 5e-4 * rng.standard_normal(m.ndof)


def device_nl(hip, name, matname, loaded):
    """fstr_StiffMatrix (+ AddBC) and the internal force of fstr_UpdateNewton at the zero state or a small loaded one."""
    import test_oracle_nl as T
    from frontistr_amd import fstr
    mat = T.materials()[matname]
    m = mesh(name)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(ctx, m.coord, m.conn, fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden,
                                                                 plconst=mat.plconst, table=mat.table if mat.table.size else None,
                                                                 nlgeom_flag=mat.nlgeom))
    if loaded:
        st, u, du = nl_state(m, mat.plastic)
        solid.set_state(dict(st, unode=u, dunode=du), latch=0)
    fstr.fstr_StiffMatrix(solid, bc_of(m))
    ctx.download_matrix(hecMAT)
    hecMAT.X[:] = 0.0
    ctx.upload(hecMAT, what=hip.FX_UP_X)
    fstr.fstr_UpdateNewton(solid)
    q = solid.get_state(("qforce",))["qforce"]
    ctx.close()
    return hecMAT, q


def compute_all(path):
    """Every device result of this module under the scatter path of this process, into one .npz."""
    from frontistr_amd import hecmw as hip
    out = {}
    for key, name, eo, variant in linear_cases():
        mat = device_linear(hip, name, eo, variant)
        for k in ("D", "AL", "AU", "B"):
            out["%s/%s" % (key, k)] = np.array(getattr(mat, k))
    for name in NL_MESHES:
        for matname in NL_MATS:
            for loaded in (False, True):
                key = "nl-%s-%s-%d" % (name, matname, loaded)
                mat, q = device_nl(hip, name, matname, loaded)
                for k in ("D", "AL", "AU"):
                    out["%s/%s" % (key, k)] = np.array(getattr(mat, k))
                out[key + "/qforce"] = q
    np.savez(path, **out)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """path -> results.  The default path runs here (twice: it must be bitwise reproducible); every other path in its own
    fresh child, one after another.  A child that dies by a signal or times out fails the module at once."""
    tmp = tmp_path_factory.mktemp("asm_paths")
    compute_all(str(tmp / "default.npz"))
    compute_all(str(tmp / "default_again.npz"))
    for path, env in PATHS.items():
        if env is None:
            continue
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_assembly_meshes as T; T.compute_all(%r)" % (
            HERE, ROOT, str(tmp / (path + ".npz")))
        try:
            p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True, timeout=600)
        except subprocess.TimeoutExpired:
            pytest.fail("scatter path %s: child timed out" % path)
        if p.returncode != 0:
            pytest.fail("scatter path %s: child exited with %d\n%s" % (path, p.returncode, p.stdout[-3000:]))
    return {p: dict(np.load(str(tmp / (p + ".npz")))) for p in list(PATHS) + ["default_again"]}


_ORACLE_LINEAR = {}


def oracle_linear(oracle, name, eo, variant):
    key = (name, eo, variant)
    if key not in _ORACLE_LINEAR:
        m = mesh(name)
        conn = subset_of(m) if variant == "subset" else m.conn
        sec = sections_of(m) if variant == "sections" else None
        _ORACLE_LINEAR[key] = oracle.assemble(eo, m.coord, conn, E, NU, bc=bc_of(m), load=m.load(), sections=sec)
    return _ORACLE_LINEAR[key]


def dense(NP, indexL, itemL, indexU, itemU, D, AL, AU):
    M = np.zeros((3 * NP, 3 * NP))
    D, AL, AU = D.reshape(-1, 3, 3), AL.reshape(-1, 3, 3), AU.reshape(-1, 3, 3)
    for i in range(NP):
        M[3 * i:3 * i + 3, 3 * i:3 * i + 3] = D[i]
        for j in range(indexL[i], indexL[i + 1]):
            M[3 * i:3 * i + 3, 3 * (itemL[j] - 1):3 * itemL[j]] = AL[j]
        for j in range(indexU[i], indexU[i + 1]):
            M[3 * i:3 * i + 3, 3 * (itemU[j] - 1):3 * itemU[j]] = AU[j]
    return M


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("key,name,eo,variant", [pytest.param(*c, id=c[0]) for c in linear_cases()])
def test_linear_assembly_vs_oracle(results, oracle, path, key, name, eo, variant):
    r = results[path]
    A = oracle_linear(oracle, name, eo, variant)
    scale = np.abs(A.D).max()
    assert np.abs(r[key + "/B"] - A.B).max() <= 1e-12 * max(np.abs(A.B).max(), 1.0)
    if variant == "subset":                                   # the device profile is the whole mesh's: compare dense images
        m = mesh(name)
        iL, jL, iU, jU = oracle.mat_con(m.n_node, m.conn)
        got = dense(m.n_node, iL, jL, iU, jU, r[key + "/D"], r[key + "/AL"], r[key + "/AU"])
        want = dense(m.n_node, A.indexL, A.itemL, A.indexU, A.itemU, A.D, A.AL, A.AU)
        assert np.abs(got - want).max() <= 1e-12 * scale
        return
    for k in ("D", "AL", "AU"):
        err = np.abs(r["%s/%s" % (key, k)] - getattr(A, k)).max()
        assert err <= 1e-12 * scale, "%s %s: %.3e relative" % (path, k, err / scale)


@pytest.mark.parametrize("key,name,eo,variant", [pytest.param(*c, id=c[0]) for c in linear_cases()])
def test_scatter_paths_agree(results, key, name, eo, variant):
    """Where the colouring succeeds, default twice, FX_ASM_FIRST=0 and FX_ASM_MAP=0 add the same contributions in the same colour
    order: the same bits, collapsed elements included (where it fails, every path is the atomic one).  The atomic paths agree to
    rounding."""
    d = results["default"]
    for k in ("D", "AL", "AU", "B"):
        kk = "%s/%s" % (key, k)
        if coloured(name):
            assert np.array_equal(d[kk], results["default_again"][kk]), k
            for p in ("first0", "map0"):
                assert np.array_equal(d[kk], results[p][kk]), (p, k)
        # coloured against atomic: 1e-13.  Where the colouring fails both are atomic, in run-dependent orders: the hub rows of
        # pie72x2x3 sum 144 contributions per block, so they are held to the oracle bound instead
        tol = 1e-13 if coloured(name) else 1e-12
        scale = np.abs(d[key + "/D"]).max()
        for p in ("atomic", "atomic_map0"):
            assert np.abs(d[kk] - results[p][kk]).max() <= tol * max(scale, 1.0), (p, k)


_ORACLE_NL = {}


def oracle_nl(oracle, name, matname, loaded):
    key = (name, matname, loaded)
    if key not in _ORACLE_NL:
        import test_oracle_nl as T
        mat = T.materials()[matname]
        m = mesh(name)
        model = oracle.NonlinearModel(mat, m.coord, m.conn)
        if loaded:
            st, u, du = nl_state(m, mat.plastic)
            model.state.update(st)
            model.unode[:], model.dunode[:] = u, du
        for a in (model.m.D, model.m.AL, model.m.AU):
            a[:] = 0.0
        model.m.B = np.zeros(3 * m.n_node)
        model.stiffness()
        model.add_bc(*bc_of(m))
        model.update()
        _ORACLE_NL[key] = (model.m.D.copy(), model.m.AL.copy(), model.m.AU.copy(), model.qforce.copy())
    return _ORACLE_NL[key]


@pytest.mark.parametrize("path", ["default", "first0", "map0", "atomic", "atomic_map0"])
@pytest.mark.parametrize("loaded", [False, True], ids=["zero_state", "loaded_state"])
@pytest.mark.parametrize("matname", NL_MATS)
@pytest.mark.parametrize("name", NL_MESHES)
def test_nonlinear_tangent_and_internal_force_vs_oracle(results, oracle, path, name, matname, loaded):
    r = results[path]
    key = "nl-%s-%s-%d" % (name, matname, loaded)
    D, AL, AU, q = oracle_nl(oracle, name, matname, loaded)
    scale = np.abs(D).max()
    for k, want in (("D", D), ("AL", AL), ("AU", AU)):
        err = np.abs(r["%s/%s" % (key, k)] - want).max()
        assert err <= 1e-11 * scale, "%s %s: %.3e relative" % (path, k, err / scale)
    if loaded:
        assert np.abs(r[key + "/qforce"] - q).max() <= 1e-11 * np.abs(q).max()
    else:
        assert np.abs(r[key + "/qforce"]).max() == 0.0 and np.abs(q).max() == 0.0
    if coloured(name) and path in COLOURED_PATHS:
        for k in ("D", "AL", "AU"):
            assert np.array_equal(r["%s/%s" % (key, k)], results["default_again"]["%s/%s" % (key, k)]), k


@pytest.mark.parametrize("name", ["pie24x2x2", "pie33x1x2", "wedge1", "pie7x3x1", "cube9_renum"])
def test_linear_stress_update_vs_oracle(oracle, name):
    from frontistr_amd import hecmw as hip
    m = mesh(name)
    u = 1e-3 * np.sin(0.7 * np.arange(3 * m.n_node) + 0.2)
    for elemopt in (1, 2, 3):
        ctx = hip.SolverContext()
        s, t, q, ms = ctx.update_c3d8_linear(m.coord, m.conn, E, NU, u, elemopt=elemopt)
        ctx.close()
        so, to, qo = oracle.update_linear(elemopt, m.coord, m.conn, E, NU, u)
        assert np.abs(s - so).max() <= 1e-11 * np.abs(so).max() and np.abs(t - to).max() <= 1e-11 * np.abs(to).max()
        assert np.abs(q - qo).max() <= 1e-11 * np.abs(qo).max()


@pytest.mark.parametrize("meth,pc", [(1, 1), (2, 10)])
@pytest.mark.parametrize("name", ["pie24x2x2", "pie72x2x3"])
def test_pie_solve_vs_oracle(hip, oracle, name, meth, pc):
    """The device-assembled pie solved on the device against the oracle's solve of the oracle's system (bounds of
    test_unstructured_hex_mesh_vs_oracle).  The slivers at the axis make pie72x2x3 far worse conditioned than the cubes: two
    BiCGSTAB solutions of it that both meet TOL 1e-8, from matrices equal to rounding, were measured 2.2e-6 apart (relative), so that
    one case is held to 1e-5; a tighter TOL does not help, it lets the iteration counts drift apart instead."""
    from oracle.refrun import default_params
    m = mesh(name)
    A = oracle.assemble(1, m.coord, m.conn, E, NU, bc=bc_of(m), load=m.load())
    I, R = default_params(method=meth, precond=pc)
    o = oracle.solve_iterative(A, I, R, nthreads=4)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.elem_node_item = m.conn.ravel()
    mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(mat, what=hip.FX_UP_PROFILE)
    ctx.assemble_c3d8(m.coord, m.conn, E, NU, elemopt=1, load=m.load(), bc=bc_of(m))
    mat.Iarray[0] = 10000; mat.Iarray[1] = meth; mat.Iarray[2] = pc
    assert ctx.solve_resident(mat) == 0 and o["code"] == 0
    ctx.download_x(mat)
    k = min(10, len(ctx.history), len(o["history"]))
    assert np.all(np.abs(ctx.history[:k] - o["history"][:k]) <= 1e-9 * o["history"][:k])
    tol_it = {1: 1, 2: 0.15 * o["iter"]}[meth]
    assert abs(ctx.info.iterations - o["iter"]) <= max(2, tol_it)
    xtol = 1e-5 if (name, meth) == ("pie72x2x3", 2) else 1e-7
    assert np.abs(mat.X - o["X"]).max() < xtol * np.abs(o["X"]).max()
    ctx.close()
