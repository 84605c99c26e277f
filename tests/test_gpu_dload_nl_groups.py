"""The host code between a caller's !DLOAD list and the load kernels on a nonlinear context (fx_nl_set_dload, nl_parts_to_host,
nl_dload_rebuild; csrc/fx_dload.h, csrc/fx_nonlinear_host.h): the resident GL against dload_ref.assemble on every family of
nl_shapes.FAMILIES as a single-type context, and on group contexts (mixed_nl_ref.gpu_case) in the caller's group numbering, the
`empty_middle` variant included.  The kernels themselves are tests/test_gpu_dload.py's business.

Single-type contexts: the skewed 3^3 meshes (27 hexahedra, 54 wedges, 162 tetrahedra; the quadratic ones curved), two materials on
the (arange * 7 // 3) % 2 pattern that belong to different kernel groups, so that nl_part_lists reorders the elements -- ELASTIC
TOTALLAG beside Mises UPDATELAG; F-bar: INFINITE beside TOTALLAG -- with densities 0.4 and 1.1.  The list: pressure on the sides
z = 3 and x = 3 (wedges: triangles and quadrilaterals), GRAV on all elements, CENT on every third, one BX entry named twice, one
held BZ entry.  unode and dunode: a random gradient of 3 % / 2 % plus noise of 0.01 per node on a mesh of size 3.

Bounds: GL is summed with atomics, in another order than the restatement's: 1e-11 of the largest entry of the restatement's GL, the
bound of test_gpu_dload*.py.  Where GL is not rebuilt (no list; no follower load) it is compared bit for bit, and so are two
rebuilds from the same inputs: the resident list is launched colour by colour, which fixes the order of the sums.  fx_nl_snapshot keeps the quadrature-point history and
leaves unode to the host (include/fistr_hip.h), so the cutback check hands unode back with set_state, as the host's routine does,
before it asks for the GL of the saved state bit for bit.

Group contexts: meshes "n3" (orders 1 and 2) and "n2r" (orders 1 and 2), the three group lists of mixed_nl_ref.VARIANTS, once
with the 361 group as F-bar; the list is built with fstr.dload_faces over the caller's list (mixed_nl_ref.top_side_dload)."""
import functools

import numpy as np
import pytest

import dload_ref as R
import mixed_nl_ref as M
import nl_shapes as S
from oracle.refrun import Material

pytestmark = pytest.mark.gpu
RHO = (0.4, 1.1)
FACTOR = 0.7
BOUND = 1e-11
GRAV = (9.8, (0.2, 0.0, -1.0))
CENT = (3.0, (1.5, 1.5, 0.0), (0.0, 0.1, 1.0))


def materials(fbar):
    """the two sections, in different kernel groups (nl_shapes.material_group): 1 and 2, F-bar 0 and 1"""
    if fbar:        # UPDATELAG is refused on F-bar elements
        return [Material(1000.0, 0.3, nlgeom=M.INFINITE), Material(1500.0, 0.25, nlgeom=M.TOTALLAG)]
    return [Material(1000.0, 0.3, nlgeom=M.TOTALLAG),
            Material(1000.0, 0.3, plastic=True, harden=0, plconst=(20.0, 100.0, 0.0), nlgeom=M.UPDATELAG)]


def two_sections(n_elem):
    return (1 + (np.arange(n_elem) * 7 // 3) % 2).astype(np.int32)


def displacements(coord, seed):
    """unode, dunode: a few percent of the mesh size"""
    rng = np.random.default_rng(seed)
    x = np.asarray(coord)
    U = x @ (rng.uniform(-1, 1, (3, 3)) * 0.03).T + rng.uniform(-1, 1, x.shape) * 0.01
    dU = x @ (rng.uniform(-1, 1, (3, 3)) * 0.02).T + rng.uniform(-1, 1, x.shape) * 0.01
    return np.ascontiguousarray(U.ravel()), np.ascontiguousarray(dU.ravel())


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _close(got, want, tag):
    err = _rel(got, want)
    print("%s: %.3e (bound %.1e)" % (tag, err, BOUND))
    assert err <= BOUND, "%s: %.3e" % (tag, err)


def _differ(a, b, tag):
    """the two restated vectors are far enough apart for the comparison to see the wrong one"""
    d = np.abs(a - b).max() / np.abs(a).max()
    assert d > 1e-3, "%s: the two configurations differ by %.3e only" % (tag, d)


def _begin(hip, solid, cload):
    cl = np.ascontiguousarray(cload, dtype=np.float64)
    hip._chk(hip.lib().fx_nl_begin_substep(solid.ctx.h, hip._ptr(cl)))
    return solid.get_load()


def _update_at(hip, solid, dunode):
    du = np.ascontiguousarray(dunode, dtype=np.float64)
    hip._chk(hip.lib().fx_nl_update_at(solid.ctx.h, hip._ptr(du), None, None))
    return solid.get_load()


def _refused(solid, dl, rho, *texts):
    from frontistr_amd.hecmw import HecmwSolverError
    with pytest.raises(HecmwSolverError) as info:
        solid.set_dload(dl, rho, follow=True)
    msg = str(info.value)
    print("refused:", msg)
    for t in texts:
        assert t in msg, (t, msg)


# ---- single-type contexts ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_case(fam):
    """-> dict of the mesh, sections, list and displacements of one family, and the restated vectors (made once, read only)"""
    from frontistr_amd import fstr
    et = S.family_type(fam)
    m = S.mesh_of("cube3" if et == 361 else "%d3" % et)
    ne = m.conn.shape[0]
    em = two_sections(ne)
    plain = [(et, m.conn)]
    faces = fstr.dload_faces(m.coord, plain, m.coord[:, 2] == 3.0) + fstr.dload_faces(m.coord, plain, m.coord[:, 0] == 3.0)
    dl = fstr.tDload()
    for g, e, f in faces:
        dl.pressure(g, [e], f, 2.0)
    dl.gravity(0, np.arange(ne), *GRAV)
    dl.centrifugal(0, np.arange(0, ne, 3), *CENT)
    dl.body(0, [1], "BX", 5.0)
    dl.body(0, [1], "BX", 5.0)
    dl.body(0, [ne - 1], "BZ", -40.0, held=True)
    shapes = [len(fstr.tDload.SUBFACE[et][f - 1]) for _, _, f in faces]
    counts = dict(tri_entries=sum(s in (3, 6) for s in shapes), quad_entries=sum(s in (4, 8) for s in shapes), body_entries=3,
                  grav_entries=ne, cent_entries=len(range(0, ne, 3)))
    if et in (351, 352):
        assert counts["tri_entries"] and counts["quad_entries"]
    U, dU = displacements(m.coord, 5 + et)
    cload = np.sin(np.arange(3 * m.n_node) * 0.23)
    groups = [(et, m.conn, None, em)]
    want = lambda factor, disp, lst=None: cload + R.assemble(m.coord, groups, RHO, dl.arrays() if lst is None else lst, factor=factor, disp=disp)
    # a second list: other values, no CENT, nothing held
    dl2 = fstr.tDload()
    for g, e, f in faces[::2]:
        dl2.pressure(g, [e], f, -1.5)
    dl2.gravity(0, np.arange(1, ne, 2), 4.0, (1.0, 0.5, 0.0))
    c = dict(et=et, m=m, em=em, dl=dl, dl2=dl2, counts=counts, U=U, dU=dU, cload=cload, faces=faces,
             follow=want(FACTOR, U), fixed=want(FACTOR, None), updated=want(FACTOR, U + dU), half=want(0.5 * FACTOR, U),
             second=want(FACTOR, U, dl2.arrays()))
    unheld = dl.arrays()[:4] + (None,)
    c["half_unheld"] = want(0.5 * FACTOR, U, unheld)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _family_context(hip, fam, c):
    from frontistr_amd import fstr
    import test_gpu_mixed_nonlinear as MT
    m, et = c["m"], c["et"]
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    mats = [MT._fmat(x) for x in materials(fam == "361f")]
    make = lambda: fstr.fstr_solid(ctx, m.coord, m.conn, mats, elem_mat=c["em"], etype=et, elemopt=4 if fam == "361f" else 2)
    return ctx, make(), make


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_resident_load_vector_of_a_family(hip, fam):
    """begin with and without the follower load, after an update, the factor"""
    c = family_case(fam)
    U, dU, cload, dl = c["U"], c["dU"], c["cload"], c["dl"]
    _differ(c["follow"], c["fixed"], "coord + unode against coord")
    _differ(c["updated"], c["follow"], "coord + unode + dunode against coord + unode")
    _differ(c["half"], c["half_unheld"], "the held entry")
    ctx, solid, _ = _family_context(hip, fam, c)
    try:
        solid.set_state({"unode": U})
        assert np.array_equal(_begin(hip, solid, cload), cload), "no list: the nodal load alone"
        solid.set_dload(dl, RHO, follow=True)
        solid.set_dload_factor(FACTOR)
        stats = ctx.dload_stats()
        assert {k: stats[k] for k in c["counts"]} == c["counts"]
        _close(_begin(hip, solid, cload), c["follow"], "%s begin, follow" % fam)
        # the stress update: GL on coord + unode + dunode
        _close(_update_at(hip, solid, dU), c["updated"], "%s after the update, follow" % fam)
        # the factor: the held entry keeps its whole value
        solid.set_dload_factor(0.5 * FACTOR)
        _close(_begin(hip, solid, cload), c["half"], "%s begin, half the factor" % fam)
        solid.set_dload_factor(FACTOR)
        # FOLLOW=NO: on coord at begin, and the update leaves GL alone
        solid.set_dload(dl, RHO, follow=False)
        fixed = _begin(hip, solid, cload)
        _close(fixed, c["fixed"], "%s begin, fixed" % fam)
        assert np.array_equal(_update_at(hip, solid, dU), fixed), "FOLLOW=NO: the update changed GL"
    finally:
        ctx.close()


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_cutback_gives_the_load_vector_of_the_saved_state(hip, fam):
    """fstr_cutback_save, an update and a commit, fstr_cutback_load, begin: GL is that of the saved state -- to 1e-11 of the
    restatement, and bit for bit the GL of the first begin on that state; two begins in a row give the same bits as well.

    This holds because the resident list is launched colour by colour (dload_colour, csrc/fx_dload.h): no two entries of a launch
    share a node, so every entry of GL is summed in the order of the launches.  With one launch per batch, the atomics of several
    workgroups met in the hardware's order, and all seven families missed the second assertion by one to three units in the last
    place (4e-16 to 2.7e-15 on entries of 2.8 to 11.2), as did two begins in a row."""
    from frontistr_amd import fstr
    c = family_case(fam)
    U, dU, cload, dl = c["U"], c["dU"], c["cload"], c["dl"]
    ctx, solid, _ = _family_context(hip, fam, c)
    try:
        solid.set_dload(dl, RHO, follow=True)
        solid.set_dload_factor(FACTOR)
        solid.set_state({"unode": U})
        first = _begin(hip, solid, cload)
        _close(first, c["follow"], "%s first begin" % fam)
        second = _begin(hip, solid, cload)
        print("%s two begins in a row: largest difference %.3e" % (fam, np.abs(second - first).max()))
        assert np.array_equal(second, first), "two begins in a row on an untouched state differ"
        fstr.fstr_cutback_save(solid)
        _update_at(hip, solid, dU)
        fstr.fstr_UpdateState(solid)
        assert np.array_equal(solid.get_state(("unode",))["unode"], U + dU)
        _close(_begin(hip, solid, cload), c["updated"], "%s begin after the commit" % fam)
        fstr.fstr_cutback_load(solid)
        solid.set_state({"unode": U})       # fstr_cutback_load's own line for unode: the snapshot holds the point history
        again = _begin(hip, solid, cload)
        _close(again, c["follow"], "%s begin after the cutback" % fam)
        print("%s begin after the cutback against the first begin: largest difference %.3e of %.3e" % (fam, np.abs(again - first).max(), np.abs(first).max()))
        assert np.array_equal(again, first), "the GL of the saved state is not the first begin's bit for bit"
    finally:
        ctx.close()


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_lists_replace_each_other_and_refusals_change_nothing(hip, fam):
    from frontistr_amd import fstr
    c = family_case(fam)
    U, cload, dl, et = c["U"], c["cload"], c["dl"], c["et"]
    ne = c["m"].conn.shape[0]
    ctx, solid, make = _family_context(hip, fam, c)
    try:
        solid.set_state({"unode": U})
        solid.set_dload_factor(FACTOR)
        solid.set_dload(dl, RHO, follow=True)
        before = _begin(hip, solid, cload)
        _close(before, c["follow"], "%s first list" % fam)
        # refused lists: the one in force stays
        nf = len(fstr.tDload.SUBFACE[et])
        _refused(solid, fstr.tDload().pressure(0, [0], 1, 1.0).pressure(0, [2], nf + 1, 1.0), RHO,
                 "entry 2 (group 1)", "TYPE=%d has no LTYPE %d" % (et, 10 * (nf + 1)))
        first2 = int(np.flatnonzero(c["em"] == 2)[0])
        _refused(solid, fstr.tDload().gravity(0, np.arange(ne), *GRAV), RHO[:1], "entry %d (group 1)" % (first2 + 1), "material id out of range")
        _refused(solid, fstr.tDload().body(0, [0, ne], "BY", 1.0), None, "entry 2", "element %d is not in group 1" % ne)
        _refused(solid, fstr.tDload().body(1, [0], "BY", 1.0), None, "entry 1", "group out of range")
        _refused(solid, fstr.tDload().gravity(0, [0], *GRAV), None, "entry 1 (group 1)", "GRAV and CENT need rho")
        assert {k: ctx.dload_stats()[k] for k in c["counts"]} == c["counts"]
        after = _begin(hip, solid, cload)
        _close(after, c["follow"], "%s after the refusals" % fam)
        assert np.array_equal(after, before), "GL changed over the refused lists"
        # a second list replaces the first
        solid.set_dload(c["dl2"], RHO, follow=True)
        _differ(c["second"], c["follow"], "the two lists")
        _close(_begin(hip, solid, cload), c["second"], "%s second list" % fam)
        assert ctx.dload_stats()["cent_entries"] == 0 and ctx.dload_stats()["grav_entries"] == len(range(1, ne, 2))
        # cleared: the nodal load alone
        solid.set_dload(None)
        assert np.array_equal(_begin(hip, solid, cload), cload)
        # a fresh context on the same fx_context forgets the list
        solid.set_dload(dl, RHO, follow=True)
        fresh = make()
        fresh.set_state({"unode": U})
        assert np.array_equal(_begin(hip, fresh, cload), cload), "a fresh fx_nl_init kept the list"
    finally:
        ctx.close()


# ---- group contexts ------------------------------------------------------------------------------------------------------------------
GROUP_CASES = [pytest.param(mesh, order, variant, False, id="%s-o%d-%s" % (mesh, order, variant))
               for mesh, order in (("n3", 1), ("n3", 2), ("n2r", 1), ("n2r", 2)) for variant in M.VARIANTS]
GROUP_CASES.append(pytest.param("n3", 1, "mesh_order", True, id="n3-o1-mesh_order-fbar"))


@pytest.mark.parametrize("mesh,order,variant,fbar", GROUP_CASES)
def test_resident_load_vector_of_a_group_context(hip, mesh, order, variant, fbar):
    """The list names groups by the caller's positions (an empty group keeps its number): begin with and without the follower
    load and after an update against the restatement on the caller's group list."""
    from frontistr_amd import fstr
    import test_gpu_mixed_nonlinear as MT
    mats = materials(fbar)
    m, groups, _, _, _ = M.gpu_case(mesh, order, variant, mats, True, history=False)
    if fbar:
        assert groups[0][0] == 361
        groups[0] = (361, groups[0][1], 4, groups[0][3])
    U, dU = displacements(m.coord, 40 + order)
    cload = np.cos(np.arange(3 * m.n_node) * 0.31)
    dl = M.top_side_dload(m, groups, 2.0, GRAV, CENT)
    lst = dl.arrays()
    named = sorted(set(lst[0].tolist()))
    assert named == [g for g, G in enumerate(groups) if G[1].shape[0]], "the list names every group that holds an element"
    shapes = {len(fstr.tDload.SUBFACE[groups[g][0]][lt // 10 - 1]) for g, lt in zip(lst[0], lst[2]) if lt >= 10}
    assert shapes == ({3, 4} if order == 1 else {6, 8}), "triangles and quadrilaterals on the top side"
    want = lambda disp: cload + R.assemble(m.coord, groups, RHO, lst, factor=FACTOR, disp=disp)
    follow, fixed, updated = want(U), want(None), want(U + dU)
    _differ(follow, fixed, "coord + unode against coord")
    _differ(updated, follow, "coord + unode + dunode against coord + unode")
    tag = "%s order %d %s%s" % (mesh, order, variant, " F-bar" if fbar else "")
    ctx, hecMAT, solid = MT._solid(hip, m, groups, mats)
    try:
        solid.set_state({"unode": U})
        solid.set_dload_factor(FACTOR)
        assert np.array_equal(_begin(hip, solid, cload), cload)
        if variant == "empty_middle":       # refused before the list below is in force: the empty group has no element
            assert groups[1][1].shape[0] == 0
            _refused(solid, fstr.tDload().body(1, [0], "BX", 1.0), None, "entry 1", "element 0 is not in group 2")
            _refused(solid, fstr.tDload().body(len(groups), [0], "BX", 1.0), None, "entry 1", "group out of range")
            assert np.array_equal(_begin(hip, solid, cload), cload)
        solid.set_dload(dl, RHO, follow=True)
        stats = ctx.dload_stats()
        assert stats["grav_entries"] == m.n_elem and stats["tri_entries"] + stats["quad_entries"] == int((lst[2] >= 10).sum())
        _close(_begin(hip, solid, cload), follow, tag + " begin, follow")
        _close(_update_at(hip, solid, dU), updated, tag + " after the update, follow")
        solid.set_dload(dl, RHO, follow=False)
        got = _begin(hip, solid, cload)
        _close(got, fixed, tag + " begin, fixed")
        assert np.array_equal(_update_at(hip, solid, dU), got), "FOLLOW=NO: the update changed GL"
        if variant == "empty_middle":       # message of an entry behind the gap: the caller's number, 1-based
            last = len(groups) - 1
            _refused(solid, fstr.tDload().pressure(last, [0], 7, 1.0), None, "entry 1 (group %d)" % (last + 1), "TYPE=%d has no LTYPE 70" % groups[last][0])
            _close(_begin(hip, solid, cload), fixed, tag + " after the refusal")
    finally:
        ctx.close()
