"""tests/mixed_nl_ref.py, the restatement of the nonlinear loop over element groups, on the CPU:

- with one group it reproduces the single-type models exactly (tet_nl_ref, c3_nl_ref, oracle.pyoracle.nl_elements);
- the latch crosses groups: the stress update of a mesh whose tetrahedra are elastoplastic latches the tangent of the
  elastoplastic hexahedra, and the C oracle's own static latch follows the model's whatever other callers left in it;
- the 1 % cap of test_gpu_mixed_nonlinear.py's two-tier UPDATELAG rule: on that test's UPDATELAG inputs the restatement alone,
  with the nodes of every STF_C3 element summed in two orders, stays inside it (the share is printed).
"""
import numpy as np
import pytest

import c3_nl_ref as CN
import mixed_nl_ref as M
import tet_nl_ref as T
from frontistr_amd.mesh import CubeMesh, solid_mesh
from oracle.refrun import Material

E0, NU0 = 206900.0, 0.29
MISES = lambda nlgeom: Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=nlgeom)


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    from oracle import pyoracle
    pyoracle.build()


@pytest.mark.parametrize("etype,single", [(341, T), (352, CN)])
def test_one_group_is_the_single_type_model(etype, single):
    m = solid_mesh(2, etype, skew=0.1)
    mat = MISES(M.UPDATELAG)
    unode, dunode, st = single.random_case(etype, mat, m, 17)
    ref = single.Model(etype, m.coord, m.conn, mat)
    ref.st = {k: v.copy() for k, v in st.items()}
    ref.unode[:], ref.dunode[:] = unode, dunode
    mod = M.Model(m.coord, [(etype, m.conn, 2, None)], mat)
    mod.set_flat(st)
    mod.unode[:], mod.dunode[:] = unode, dunode
    assert np.array_equal(mod.element_tangents()[0], ref.element_tangents())
    assert np.array_equal(mod.stiffness(), ref.stiffness())
    assert np.array_equal(mod.element_update()[0], ref.element_update())
    for k in M.STATE6 + M.STATE1:
        assert np.array_equal(mod.flat(k), ref.st[k].ravel()), k
    assert mod.latch == ref.latch == 1
    assert np.array_equal(mod.dstress[0], ref.dstress)
    assert np.array_equal(mod.element_tangents()[0], ref.element_tangents())
    assert np.array_equal(mod.update(), ref.update())
    mod.commit(); ref.commit()
    for k in M.STATE6 + M.STATE1:
        assert np.array_equal(mod.flat(k), ref.st[k].ravel()), k


def test_one_group_of_hexahedra_is_the_oracle():
    from oracle import pyoracle as po
    m = CubeMesh(2, skew=0.1)
    mat = MISES(M.UPDATELAG)
    unode, dunode, st = M.random_case(m, [(361, m.conn, 2, None)], mat, 11)
    shaped = {k: v.reshape((m.n_elem, 8, 6) if k in M.STATE6 else (m.n_elem, 8)) for k, v in st.items()}
    ke0, qf, ke1, ost = po.nl_elements(mat, m.coord, m.conn, unode, dunode, shaped)
    mod = M.Model(m.coord, [(361, m.conn, 2, None)], mat)
    mod.set_flat(st)
    mod.unode[:], mod.dunode[:] = unode, dunode
    assert np.array_equal(mod.element_tangents()[0], ke0)
    assert np.array_equal(mod.element_update()[0], qf)
    for k in M.STATE6 + M.STATE1:
        assert np.array_equal(mod.flat(k), ost[k].ravel()), k
    assert np.array_equal(mod.element_tangents()[0], ke1)
    assert np.abs(ke1 - ke0).max() > 1e-3 * np.abs(ke0).max()      # the latch took the elastoplastic matrix away


def test_the_latch_crosses_groups():
    from oracle import pyoracle as po
    mats = [MISES(M.UPDATELAG), MISES(M.TOTALLAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)]
    mesh = M._mesh("n2", 1)
    o = mesh.elem_offsets
    em = np.concatenate([np.full(o[1] - o[0], 2), np.full(o[2] - o[1], 3), np.full(o[3] - o[2], 1)]).astype(np.int32)
    groups = M.group_list(mesh, "mesh_order", em)       # hexahedra Mises TOTALLAG, wedges ELASTIC, tetrahedra Mises UPDATELAG
    unode, dunode, st = M.random_case(mesh, groups, mats, 3)
    mod = M.Model(mesh.coord, groups, mats)
    mod.set_flat(st)
    mod.unode[:], mod.dunode[:] = unode, dunode
    assert (mod.parts[0]["st"]["istat"] != 0).any()
    before = mod.element_tangents()
    M._set_c_latch(1)                                   # whatever another caller left in the C oracle's static
    again = mod.element_tangents()
    for a, b in zip(before, again):
        assert np.array_equal(a, b)
    hex_state = {k: v.copy() for k, v in mod.parts[0]["st"].items()}
    mod.element_update()
    assert mod.latch == 1
    mod.parts[0]["st"] = hex_state                      # the hexahedra as before the update: only the latch differs now
    po.nl_reset_latch()
    after = mod.element_tangents()
    elastic = M.Model(mesh.coord, groups, [Material(E0, NU0, nlgeom=x.nlgeom) if x.plastic else x for x in mats])
    elastic.set_flat({k: mod.flat(k) for k in M.STATE6 + M.STATE1})
    elastic.unode[:], elastic.dunode[:] = unode, dunode
    want = elastic.element_tangents()
    assert np.abs(after[0] - before[0]).max() > 1e-3 * np.abs(before[0]).max()
    assert np.array_equal(after[0], want[0])
    assert np.array_equal(after[1], want[1]) and np.array_equal(after[2], want[2])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mesh", M.MESHES)
def test_updated_lagrange_single_precision_share(mesh, order):
    """The share of the stress components of the STF_C3 groups that two orders of summation put on different single-precision
    neighbours (`real()` of the UPDATELAG stress increment), on the inputs of the GPU test's UPDATELAG cases."""
    import test_gpu_mixed_nonlinear as G
    for kind in ("bilinear", "two_sections"):
        mats, two = G.materials(kind, M.UPDATELAG)
        msh, groups, unode, dunode, st = M.gpu_case(mesh, order, "mesh_order", mats, two)
        got = []
        for od in (None, M.reverse):
            mod = M.Model(msh.coord, groups, mats)
            mod.set_flat(st)
            mod.unode[:], mod.dunode[:] = unode, dunode
            mod.element_update(od)
            got.append((np.concatenate([p["st"]["stress"].ravel() for p in mod.parts if p["etype"] != 361]),
                        max(np.abs(d).max() for d in mod.dstress)))
        (a, ds), (b, _) = got
        diff = np.abs(a - b) / ds
        share = (diff > 1.0e-11).mean()
        print("%s order %d %s: %.4f of the components differ by more than 1e-11, max %.3e (2 ulp = %.3e)"
              % (mesh, order, kind, share, diff.max(), 2.0 * 2.0 ** -23))
        assert diff.max() <= 2.0 * 2.0 ** -23
        assert share <= 0.01
