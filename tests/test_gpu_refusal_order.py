"""The order of the refusals of the entry points over element groups, with their codes and texts as the host checks of
fx_assemble_groups.h (check_group_types, check_group_elements, check_list_entry), fx_heat.h, fx_heat_bc.h, fx_dload.h and
fx_nodal_stress.h give them: a call that is wrong in two ways names the fault that comes first.  A fault that one entry point
accepts (a 361 element naming a node twice) shows as the refusal of the fault behind it.

Shapes: two elements per group.  Every call is refused before anything is uploaded, so no kernel runs here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ASC, C3D8_FIRST = "341, 342, 351, 352, 361, 362", "361, 341, 342, 351, 352, 362"
HEXES = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [5, 6, 7, 8, 9, 10, 11, 12]], dtype=np.int32)
TETS = np.array([[1, 2, 3, 5], [2, 3, 4, 6]], dtype=np.int32)
COORD = np.array([[x, y, z] for z in (0.0, 1.0, 2.0) for x, y in ((0, 0), (1, 0), (1, 1), (0, 1))], dtype=np.float64)
N = COORD.shape[0]
TEMP = np.full(N, 300.0)
I0 = np.zeros(1, dtype=np.int32)


@pytest.fixture(scope="module")
def ctx(hip):
    c = hip.SolverContext(device=0)
    yield c
    c.close()


def _collapsed(conn):
    c = conn.copy()
    c[0, 3] = c[0, 0]
    return c


def _refused(hip, code, who, text, call):
    with pytest.raises(hip.HecmwSolverError) as e:
        call()
    assert e.value.code == code and str(e.value) == "HEC-MW-SOLVER %d: %s: %s" % (code, who, text), str(e.value)


def _heat(hip, ctx, groups, ndof=1, coord=COORD, mats=None, profile_groups=None, **kw):
    from frontistr_amd.heat import heat_matrix, tHeatMaterial
    M = heat_matrix(N, profile_groups or [(361, HEXES)])[1]
    M.NDOF = ndof
    mats = [tHeatMaterial([(50.0, 0.0)])] if mats is None else mats
    return lambda: ctx.heat_assemble_groups(coord, groups, mats, M, TEMP[:coord.shape[0]], **kw)


def test_heat_assembly_refuses_in_its_order(hip, ctx):
    who, bc = "fx_heat_assemble_groups", "fx_heat_assemble_groups_bc"
    no_type = "group 1: element type 999 not supported on the device (%s)" % ASC
    # 1 types, 2 NDOF, 3 empty mesh, 4 profile size
    _refused(hip, -2, who, no_type, _heat(hip, ctx, [(999, HEXES)], ndof=3))
    _refused(hip, -2, who, "the heat matrix has NDOF = 1 (got 3)", _heat(hip, ctx, [(361, HEXES)], ndof=3, coord=np.zeros((0, 3))))
    _refused(hip, -1, who, "empty mesh", _heat(hip, ctx, [(361, HEXES)], coord=np.zeros((0, 3))))
    _refused(hip, -1, who, "mesh/profile size mismatch", _heat(hip, ctx, [(361, _collapsed(HEXES))], coord=COORD[:8]))
    # 7 materials, 8 fixed nodes, 9 the per-group loop, 10 the surface lists
    far = (I0 + 3, I0 + 5, I0 + 9, 1.0)
    _refused(hip, -1, who, "materials missing", _heat(hip, ctx, [(361, _collapsed(HEXES))], mats=[], fix=([N + 1], [0.0])))
    _refused(hip, -1, bc, "fixed node id out of range", _heat(hip, ctx, [(361, _collapsed(HEXES))], fix=([N + 1], [0.0]), dflux=far))
    dup = "group 1 (TYPE=361), element 1 names a node twice (a degenerate element)"
    _refused(hip, -1, who, dup, _heat(hip, ctx, [(361, _collapsed(HEXES))]))
    _refused(hip, -1, bc, dup, _heat(hip, ctx, [(361, _collapsed(HEXES))], dflux=far))
    # a bad node id in group 2 with a duplicate in group 1: the groups are checked one after the other
    bad = HEXES[1:].copy()
    bad[0, 2] = N + 1
    two = [(341, TETS), (361, HEXES[1:])]
    _refused(hip, -1, who, "group 1 (TYPE=341), element 1 names a node twice (a degenerate element)",
             _heat(hip, ctx, [(341, _collapsed(TETS)), (361, bad)], profile_groups=two))
    _refused(hip, -1, who, "group 2, element 1: node id out of range", _heat(hip, ctx, [(341, TETS), (361, bad)], profile_groups=two))


@pytest.mark.parametrize("kind", ["dflux", "film", "radiate"])
def test_heat_list_entry_names_group_then_element_then_face(hip, ctx, kind):
    who = "fx_heat_assemble_groups_bc"
    tail = (1.0,) if kind == "dflux" else (1.0, 300.0)
    entry = lambda g, e, f: {kind: (I0 + g, I0 + e, I0 + f) + tail}
    _refused(hip, -1, who, "%s, entry 1: group out of range" % kind, _heat(hip, ctx, [(361, HEXES)], **entry(1, 5, 9)))
    _refused(hip, -1, who, "%s, entry 1: element 5 is not in group 1" % kind, _heat(hip, ctx, [(361, HEXES)], **entry(0, 5, 9)))
    _refused(hip, -1, who, "%s, entry 1: TYPE=361 has no face 9" % kind, _heat(hip, ctx, [(361, HEXES)], **entry(0, 1, 9)))


def test_a_collapsed_hexahedron_passes_the_linear_and_the_load_checks(hip, ctx):
    bad = HEXES[1:].copy()
    bad[0, 2] = N + 1
    groups = [(361, _collapsed(HEXES[:1])), (361, bad)]
    text = "group 2, element 1: node id out of range"
    _refused(hip, -1, "fx_assemble_groups", text, lambda: ctx.assemble_groups(COORD, groups, 210000.0, 0.3))
    dl = (I0, I0, I0 + 10, np.zeros((1, 7)))
    _refused(hip, -1, "fx_dload_groups", text, lambda: ctx.dload_groups(COORD, groups, None, dl))
    _refused(hip, -1, "fx_dload_groups", "dload, entry 1: group out of range",
             lambda: ctx.dload_groups(COORD, [(361, _collapsed(HEXES))], None, (I0 + 1, I0 + 5, I0 + 90, np.zeros((1, 7)))))


def test_dload_refuses_in_its_order(hip, ctx):
    who, groups = "fx_dload_groups", [(361, HEXES)]
    dl = lambda g, e, lt: (I0 + g, I0 + e, I0 + lt, np.zeros((1, 7)))
    _refused(hip, -2, who, "group 1: element type 999 not supported on the device (%s)" % C3D8_FIRST,
             lambda: ctx.dload_groups(np.zeros((0, 3)), [(999, HEXES)], None, dl(1, 5, 90)))
    _refused(hip, -1, who, "empty mesh", lambda: ctx.dload_groups(np.zeros((0, 3)), groups, None, dl(1, 5, 90)))
    _refused(hip, -1, who, "group 1 (TYPE=341), element 1 names a node twice (a degenerate element)",
             lambda: ctx.dload_groups(COORD, [(341, _collapsed(TETS))], None, dl(1, 5, 90)))
    _refused(hip, -1, who, "dload, entry 1: group out of range", lambda: ctx.dload_groups(COORD, groups, None, dl(1, 5, 90)))
    _refused(hip, -1, who, "dload, entry 1: element 5 is not in group 1", lambda: ctx.dload_groups(COORD, groups, None, dl(0, 5, 90)))
    _refused(hip, -1, who, "dload, entry 1 (group 1): TYPE=361 has no LTYPE 90", lambda: ctx.dload_groups(COORD, groups, None, dl(0, 1, 90)))
    _refused(hip, -1, who, "dload, entry 1 (group 1): GRAV and CENT need rho", lambda: ctx.dload_groups(COORD, groups, None, dl(0, 1, 4)))


def test_linear_assembly_and_nodal_stress_name_the_type_first(hip, ctx):
    no_type = "group 1: element type 999 not supported on the device (%s)" % C3D8_FIRST
    _refused(hip, -2, "fx_assemble_groups", no_type, lambda: ctx.assemble_groups(np.zeros((0, 3)), [(999, HEXES)], 210000.0, 0.3))
    _refused(hip, -2, "fx_assemble_groups", "group 1: elemopt must be 1 (IC), 2 (B-bar) or 3 (FI)",
             lambda: ctx.assemble_groups(np.zeros((0, 3)), [(361, HEXES, 4)], 210000.0, 0.3))
    _refused(hip, -1, "fx_assemble_groups", "empty mesh", lambda: ctx.assemble_groups(np.zeros((0, 3)), [(361, _collapsed(HEXES))], 210000.0, 0.3))
    pts = np.zeros(2 * 8 * 6)
    who = "fx_nodal_stress_groups"
    _refused(hip, -2, who, no_type, lambda: ctx.nodal_stress_groups(0, [(999, HEXES)], pts, pts, principal=256))
    _refused(hip, -1, who, "empty mesh or missing point arrays", lambda: ctx.nodal_stress_groups(0, [(361, HEXES)], pts, pts, principal=256))
    _refused(hip, -1, who, "flags outside 0..255", lambda: ctx.nodal_stress_groups(N, [(361, HEXES)], pts, pts, principal=256))
    bad = HEXES.copy()
    bad[1, 2] = N + 1      # the node list is built after these checks: a bad id is named there, a node named twice is not refused
    _refused(hip, -1, who, "group 1, element 2: node id out of range", lambda: ctx.nodal_stress_groups(N, [(361, _collapsed(bad))], pts, pts))
