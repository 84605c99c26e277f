#!/usr/bin/env python3
"""Bitwise A/B of the element kernels' results between two builds of libfistr_hip.so (a refactor must not move a bit).

    ab_nl_bitwise.py --dump OUT.npz [--lib PATH]            run the nonlinear cases below in this process, write every output
    ab_nl_bitwise.py --dump-linear OUT.npz [--lib PATH]     the same for the linear case set at the end of this text
    ab_nl_bitwise.py --dump-fields OUT.npz [--lib PATH]     the same for the heat, load and stress-output case set at the end of this text
    ab_nl_bitwise.py --compare A.npz B.npz                  per array: equal bit for bit, or the first difference; exit 1 on any

Not a test: the second build (the parent commit's) is not in the repository.  Run --dump once with each library, each in a fresh
process (a few seconds), then --compare.

Cases, on the small distorted meshes of the GPU tests (hyper_ref.gpu_mesh: a handful of elements; 361 with a collapsed hexahedron):
  every type 361, 341, 342, 351, 352, 362 x group 0..6 -- ELASTIC and Mises for each NLGEOM flag, Mooney-Rivlin (group 3),
  Drucker-Prager and Mohr-Coulomb for each flag (yield_ref.gpu_case: points on both sides of the surface) --,
  a two-section context per type (Mises UPDATELAG beside ELASTIC TOTALLAG), and two fx_nl_init_groups contexts (hexahedra + wedges +
  tetrahedra, linear and quadratic) with the same two sections;
  F-bar (elemopt 4): one-group contexts for groups 0, 1 and 3 (ELASTIC INFINITE, ELASTIC TOTALLAG, Mooney-Rivlin), and one context of
  an F-bar, a B-bar and a wedge group with two sections (Mises TOTALLAG beside ELASTIC INFINITE);
  a 361 two-section context in which two hexahedra name a node twice (the collapsed-element tail of both launchers).
Outputs per case: element tangents before the first update and after it (the latch), the per-element internal forces of the update,
the state after the update and after fx_nl_commit, and D / AL / AU of the coloured scatter (fx_nl_stiffness_at, fx_download_matrix)
before and after the update.  Nodal QFORCE and the FX_ASM_ATOMIC scatter are sums of fp64 atomics in no fixed order: not compared.

Linear case set (the host path of the linear static analysis), on the small distorted meshes of test_gpu_mixed_assembly.py:
  every type through its single-type entry points, with one material and with two sections -- 361 with elemopt 1, 2, 3 and with
  a collapsed hexahedron --, and the two three-type mixed meshes through fx_assemble_groups / fx_update_groups_linear, one
  material and three sections.
Outputs per case: D / AL / AU / B after assembly without and with load and boundary conditions, strain and stress of the update
without and with a thermal view; per type the element stiffness.  A refused call is recorded by its return code.  Run it under
the default, FX_ASM_FIRST=0 and FX_ASM_MAP=0, each in its own process (the switches are read once).  QFORCE and the thermal load
vector are atomic sums: not compared.

Field case set (the host paths of heat conduction, distributed loads and stress output):
  fx_heat_assemble_groups_bc, stationary and transient, with DFLUX (faces and the body flux), FILM and RADIATE lists, and
  fx_nodal_stress_groups with every principal array, on the small distorted meshes of test_gpu_heat_bc.py (each of the six types,
  the two three-type mixed meshes) and on a 5^3 mesh of each type (more than one workgroup and more than one colour per launch);
  fx_heat_element and fx_heat_face for every type, kind and face, fx_dload_element for every type and every LTYPE it has.
  None of these adds atomically: --compare wants them equal bit for bit.  fx_dload_groups (the meshes and lists of
  test_gpu_dload.py) and fx_nl_get_load are sums of fp64 atomics: their keys end in "~atomic" and --compare holds them to that
  test's bound, 1e-11 of the largest entry.  The refusals of tests/test_gpu_refusal_order.py's kind -- a collapsed 361 element in
  the heat assembly (refused) and in fx_assemble_groups / fx_dload_groups (accepted), an unknown type with NDOF = 3, NDOF = 3 with an
  empty mesh, a bad node id behind a duplicate, a list entry of dflux, film, radiate and dload with its group, then its element, then
  its face out of range -- are recorded with code and message."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STATE = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
ETYPES = (361, 341, 342, 351, 352, 362)
E0, NU0 = 206900.0, 0.29
ATOMIC_BOUND = 1e-11      # of the largest entry: what tests/test_gpu_dload.py allows a vector summed with fp64 atomics


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("%-60s only in one file" % k)
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes():
            print("%-60s equal (%d values)" % (k, x.size))
            continue
        if k.endswith("~atomic") and x.shape == y.shape and np.abs(x - y).max() <= ATOMIC_BOUND * np.abs(y).max():
            print("%-60s within %.0e of the largest entry: %.2e (%d values)" % (k, ATOMIC_BOUND, np.abs(x - y).max() / np.abs(y).max(), x.size))
            continue
        bad.append(k)
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%-60s DIFFERS: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            continue
        xb, yb = x.ravel().view(np.uint8).reshape(x.size, -1), y.ravel().view(np.uint8).reshape(y.size, -1)
        i = int(np.flatnonzero((xb != yb).any(axis=1))[0])
        print("%-60s DIFFERS: %d of %d values, first at %d: %r against %r" % (k, int((xb != yb).any(axis=1).sum()), x.size, i,
                                                                              x.ravel()[i], y.ravel()[i]))
    print("%d arrays differ" % len(bad) if bad else "all arrays equal bit for bit (the atomic sums, if any: within their bound)")
    return 1 if bad else 0


def dump(path):
    import hyper_ref as H
    import mixed_nl_ref as M
    import yield_ref as Y
    from frontistr_amd import fstr, hecmw as hip
    from oracle.refrun import Material
    assert not os.environ.get("FX_ASM_ATOMIC"), "the atomic scatter has no fixed order"

    def fmat(mat):
        if Y.is_yield(mat):
            fm = fstr.tMaterial(mat.E, mat.nu, plastic=True, harden=0, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)
            fm.kind, fm.plconst4 = (fstr.MOHRCOULOMB if mat.kind == Y.MOHR else fstr.DRUCKERPRAGER), mat.plconst4
            return fm
        if H.kind_of(mat) == H.ARRUDA:
            return fstr.tMaterial.arruda_boyce(*mat.plconst)
        if H.kind_of(mat) == H.MOONEY:
            return fstr.tMaterial.mooney_rivlin(*mat.plconst)
        return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst,
                              table=mat.table if mat.table.size else None, nlgeom_flag=mat.nlgeom)

    out = {}

    def run(name, mesh, groups, mats, unode, dunode, st):
        """groups: [(etype, conn, elemopt, elem_mat)]; one group: the single-type context"""
        hm = hip.hecmwST_local_mesh(n_node=mesh.n_node)
        if len(groups) == 1:
            et, conn, eo, em = groups[0]
            hm.nn_elem = conn.shape[1]
            hm.elem_node_item = conn.ravel()
            hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        else:
            hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
        ctx = hip.SolverContext()
        ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
        fm = [fmat(x) for x in mats]
        if len(groups) == 1:
            solid = fstr.fstr_solid(ctx, mesh.coord, conn, fm if len(fm) > 1 else fm[0], elem_mat=em, etype=et, elemopt=eo)
        else:
            solid = fstr.fstr_solid(ctx, mesh.coord, None, fm, groups=groups)
        solid.set_state(dict(st or {}, unode=unode, dunode=dunode), latch=0)

        def tangents(tag):
            out["%s/%s/element_tangents" % (name, tag)] = solid.element_tangents()
            hip._chk(hip.lib().fx_nl_stiffness_at(ctx.h, hip._ptr(unode), hip._ptr(dunode), None))
            ctx.download_matrix(hecMAT)
            for k in ("D", "AL", "AU"):
                out["%s/%s/%s" % (name, tag, k)] = np.array(getattr(hecMAT, k))

        def state(tag):
            s = solid.get_state(STATE)
            for k in STATE:
                out["%s/%s/%s" % (name, tag, k)] = s[k]
            out["%s/%s/latch" % (name, tag)] = np.array([s["latch"]])

        tangents("before_update")
        out["%s/element_forces" % name] = solid.element_update()
        state("after_update")
        tangents("after_update")
        fstr.fstr_UpdateState(solid)
        state("after_commit")
        ctx.close()

    def single(name, etype, mesh, mats, em, unode=None, dunode=None, history=True, elemopt=2):
        groups = [(etype, mesh.conn, elemopt, em)]
        if unode is None:
            unode, dunode, st = M.random_case(mesh, groups, mats, 17, history=history)
        else:
            st = None
        run(name, mesh, groups, mats, unode, dunode, st)

    mises = lambda flag: Material(E0, NU0, plastic=True, harden=0, plconst=(450.0, 2000.0, 0.0), nlgeom=flag)
    flags = ((M.INFINITE, "infinite"), (M.TOTALLAG, "totallag"), (M.UPDATELAG, "updatelag"))
    for et in ETYPES:
        mesh = H.gpu_mesh(et)
        for flag, fname in flags:
            single("t%d_elastic_%s" % (et, fname), et, mesh, [Material(E0, NU0, nlgeom=flag)], None)
            single("t%d_mises_%s" % (et, fname), et, mesh, [mises(flag)], None)
            for family in ("drucker", "mohr"):
                m, mat, unode, dunode = Y.gpu_case(et, family, flag)
                single("t%d_%s_%s" % (et, family, fname), et, m, [mat], None, unode, dunode)
        unode, dunode = H.random_displacement(mesh.coord, 17, H.GPU_AMP)
        single("t%d_mooney" % et, et, mesh, [H.TEST_MATERIALS["mooney"]()], None, unode, dunode)
        em = (1 + (np.arange(mesh.n_elem) * 7 // 3) % 2).astype(np.int32)
        single("t%d_two_sections" % et, et, mesh, [mises(M.UPDATELAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)], em)
    for order in (1, 2):
        mats = [mises(M.UPDATELAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)]
        mesh, groups, unode, dunode, st = M.gpu_case("n3", order, "mesh_order", mats, True)
        run("groups_order%d_two_sections" % order, mesh, groups, mats, unode, dunode, st)
    mesh = H.gpu_mesh(361)
    for g, mat in ((0, Material(E0, NU0, nlgeom=M.INFINITE)), (1, Material(E0, NU0, nlgeom=M.TOTALLAG)), (3, H.TEST_MATERIALS["mooney"]())):
        unode, dunode = H.random_displacement(mesh.coord, 17, H.GPU_AMP)
        single("t361_fbar_group%d" % g, 361, mesh, [mat], None, unode, dunode, elemopt=4)
    mats = [mises(M.TOTALLAG), Material(70000.0, 0.33, nlgeom=M.INFINITE)]
    mixed = M._mesh("n3", 1)
    hexes, wedges = mixed.groups_with(2, (1 + (np.arange(mixed.n_elem) * 7 // 3) % 2).astype(np.int32))[:2]
    assert hexes[0] == 361 and wedges[0] == 351
    groups = [(361, np.ascontiguousarray(hexes[1][:2]), 4, np.ascontiguousarray(hexes[3][:2])),
              (361, np.ascontiguousarray(hexes[1][2:]), 2, np.ascontiguousarray(hexes[3][2:])), wedges]
    run("groups_fbar_bbar_wedges", mixed, groups, mats, *M.random_case(mixed, groups, mats, 17))
    conn = mesh.conn.copy()
    conn[0, 7], conn[0, 6] = conn[0, 4], conn[0, 5]      # a second collapsed hexahedron beside the mesh's own
    assert sum(len(set(c)) < 8 for c in conn.tolist()) == 2
    groups = [(361, conn, 2, (1 + (np.arange(mesh.n_elem) * 7 // 3) % 2).astype(np.int32))]
    mats = [mises(M.UPDATELAG), Material(70000.0, 0.33, nlgeom=M.TOTALLAG)]
    run("t361_two_collapsed_two_sections", mesh, groups, mats, *M.random_case(mesh, groups, mats, 17))
    np.savez(path, **out)
    print("%d arrays of %d cases written to %s (library %s)" % (len(out), len({k.split("/")[0] for k in out}), path, hip.LIBPATH))
    return 0


def dump_linear(path):
    from frontistr_amd import hecmw as hip
    from frontistr_amd.mesh import CubeMesh, MixedMesh, mesh_groups, solid_mesh
    assert not os.environ.get("FX_ASM_ATOMIC"), "the atomic scatter has no fixed order"
    out = {}

    def record(name, call):
        """call() -> {key: array}; a refusal is recorded by its code"""
        try:
            for k, v in call().items():
                out["%s/%s" % (name, k)] = np.array(v)
        except hip.HecmwSolverError as e:
            out["%s/refused" % name] = np.array([e.code])

    def case(name, m, groups, Es, nus, single):
        """single: the group goes through the single-type entry points"""
        et, conn, eo, em = groups[0]
        hm = hip.hecmwST_local_mesh(n_node=m.n_node)
        if single:
            hm.nn_elem = conn.shape[1]
            hm.elem_node_item = conn.ravel()
            mat = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        else:
            mat = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
        ctx = hip.SolverContext()
        ctx.upload(mat, what=hip.FX_UP_PROFILE)

        def assemble(load, bc):
            if not single:
                ctx.assemble_groups(m.coord, groups, Es, nus, load=load, bc=bc)
            elif et == 361:
                ctx.assemble_c3d8(m.coord, conn, Es[0], nus[0], elemopt=eo, load=load, bc=bc,
                                  sections=None if em is None else (Es, nus, em))
            else:
                ctx.assemble_c3(m.coord, conn, et, Es, nus, load=load, bc=bc, elem_mat=em)
            ctx.download_matrix(mat)
            return {k: getattr(mat, k) for k in ("D", "AL", "AU", "B")}

        def update(thermal):
            if thermal is not None or not single:
                s, t, _, _ = ctx.update_groups_linear(m.coord, groups, Es, nus, u, thermal=thermal)
            elif et == 361:
                s, t = ctx.update_c3d8_linear(m.coord, conn, Es, nus, u, elemopt=eo, elem_mat=em)[:2]
                s, t = [s], [t]
            else:
                s, t = ctx.update_c3_linear(m.coord, conn, et, Es, nus, u, elem_mat=em)[:2]
                s, t = [s], [t]
            res = {"strain%d" % g: v for g, v in enumerate(s)}
            res.update({"stress%d" % g: v for g, v in enumerate(t)})
            return res

        rng = np.random.default_rng(11)
        u = 1e-3 * rng.standard_normal(3 * m.n_node)
        temp, temp0 = 20.0 + 30.0 * rng.random(m.n_node), 20.0 + 5.0 * rng.random(m.n_node)
        record(name + "/assemble", lambda: assemble(None, None))
        record(name + "/assemble_load_bc", lambda: assemble(m.load(), m.dirichlet()))
        record(name + "/assemble_again", lambda: assemble(None, None))
        record(name + "/update", lambda: update(None))
        record(name + "/update_thermal", lambda: update((temp, temp0, 20.0, 1.2e-5 * (1.0 + np.arange(len(Es))))))
        ctx.close()

    one = {361: lambda: CubeMesh(4, skew=0.1), 341: lambda: solid_mesh(3, 341, skew=0.1),
           342: lambda: solid_mesh(2, 342, skew=0.1, curve=0.04), 351: lambda: solid_mesh(3, 351, skew=0.1),
           352: lambda: solid_mesh(2, 352, skew=0.1, curve=0.04), 362: lambda: solid_mesh(2, 362, skew=0.1, curve=0.04)}
    E1, NU1 = np.array([210000.0]), np.array([0.3])
    ES, NUS = np.array([210000.0, 70000.0, 150000.0]), np.array([0.3, 0.33, 0.25])
    for et in ETYPES:
        m = one[et]()
        variants = [("", m.conn)]
        if et == 361:
            c = m.conn.copy()
            c[3, 3], c[3, 7] = c[3, 0], c[3, 4]
            variants.append(("_collapsed", c))
        for tag, conn in variants:
            for eo in ((1, 2, 3) if et == 361 else (1,)):
                em = (1 + np.arange(m.n_elem) % 2).astype(np.int32)
                name = "t%d%s%s" % (et, tag, "_elemopt%d" % eo if et == 361 else "")
                case(name + "_one_material", m, [(et, conn, eo, None)], E1, NU1, True)
                case(name + "_two_sections", m, [(et, conn, eo, em)], ES[:2], NUS[:2], True)
        ctx = hip.SolverContext()
        ec = m.coord[m.conn[1] - 1]
        for eo in ((1, 2, 3) if et == 361 else (1,)):
            out["t%d_elemopt%d/element_stiffness" % (et, eo)] = (ctx.element_stiffness(eo, ec, 210000.0, 0.3) if et == 361 else
                                                                 ctx.element_stiffness_c3(et, ec, 210000.0, 0.3))
        ctx.close()
    for order in (1, 2):
        m = MixedMesh(2, order=order, skew=0.1, curve=0.04 if order == 2 else 0.0)
        case("mixed_order%d_one_material" % order, m, m.groups, E1, NU1, False)
        em = (1 + np.arange(m.n_elem) % 3).astype(np.int32)
        case("mixed_order%d_three_sections" % order, m, m.groups_with(elemopt=2, elem_mat=em), ES, NUS, False)
    np.savez(path, **out)
    print("%d arrays of %d cases written to %s (library %s; FX_ASM_FIRST=%s FX_ASM_MAP=%s)" % (
        len(out), len({k.split("/")[0] for k in out}), path, hip.LIBPATH, os.environ.get("FX_ASM_FIRST", "-"),
        os.environ.get("FX_ASM_MAP", "-")))
    return 0


def dump_fields(path):
    import test_gpu_dload as TD
    import test_gpu_heat as TG
    import test_gpu_heat_bc as TB
    import test_gpu_nodal_stress as TN
    import test_gpu_refusal_order as RO
    from frontistr_amd import fstr, hecmw as hip
    from frontistr_amd.heat import heat_matrix
    from test_dload_ref import skewed_element
    out = {}

    def record(name, call):
        """call() -> {key: array}; a refusal is recorded by its code and its message"""
        try:
            for k, v in call().items():
                out["%s/%s" % (name, k)] = np.array(v)
        except hip.HecmwSolverError as e:
            out["%s/refused" % name] = np.array([e.code])
            out["%s/message" % name] = np.array(str(e))

    ctx = hip.SolverContext()

    def heat(m, groups, M, beta, dtime, lists):
        temp, temp0 = TG.fields(m.coord)
        ctx.heat_assemble_groups(m.coord, groups, TG.materials(True), M, temp, temp0, beta=beta, dtime=dtime, dflux=lists[0], film=lists[1],
                                 radiate=lists[2], tzero=TB.TZERO)
        return {k: getattr(M, k).copy() for k in ("D", "AL", "AU", "B")}

    def nodal(m, groups):
        st, ss = TN.points(groups, 7)
        res = ctx.nodal_stress_groups(m.n_node, groups, st, ss, principal=255)
        return {k: getattr(res, k).copy() for k in TN.ARRAYS}

    meshes = [("small_%s" % k, TB.case_mesh(k)) for k in TG.KINDS] + [("n5_t%d" % et, TG._mesh(et, 5)) for et in TG.TYPES]
    for name, m in meshes:
        groups = [(et, conn, None, (1 + (np.arange(conn.shape[0]) % 2)).astype(np.int32)) for et, conn in TG._groups(m)]
        M = heat_matrix(m.n_node, groups)[1]
        lists = TB.lists_of(m, groups)
        for tag, beta, dtime in (("stationary", 1.0, 0.0), ("transient", 0.5, 0.37), ("stationary_again", 1.0, 0.0)):
            record("%s/heat_%s" % (name, tag), lambda: heat(m, groups, M, beta, dtime, lists))
        record("%s/nodal_stress" % name, lambda: nodal(m, [g[:2] for g in groups]))

    hmats = TG.materials(True)
    for et in TG.TYPES:
        X, _ = skewed_element(et, curve=0.07)
        nn = X.shape[0]
        tt, tt0 = 300.0 + 250.0 * np.sin(1.0 + np.arange(nn)), 250.0 + 200.0 * np.cos(2.0 + np.arange(nn))
        for dtime in (0.0, 0.25):
            ss, s0 = ctx.heat_element(et, X, tt, hmats[0], tt0=tt0, dtime=dtime)
            out["t%d/heat_element_dtime%g/ss" % (et, dtime)] = ss
            if s0 is not None:
                out["t%d/heat_element_dtime%g/s0" % (et, dtime)] = s0
        nf = len(fstr.tDload.SUBFACE[et])
        for kind in ("dflux", "film", "radiate"):
            for f in range(0 if kind == "dflux" else 1, nf + 1):
                t1, t2, nod = ctx.heat_face(et, kind, f, X, 25.0, sink=600.0, tt=tt, tzero=TB.TZERO)
                res = {"term2": t2, "nod": nod}
                if t1 is not None:
                    res["term1"] = t1
                for k, v in res.items():
                    out["t%d/heat_face_%s_%d/%s" % (et, kind, f, k)] = v
        cases = [(1, [3.0]), (2, [-2.0]), (3, [1.5]), (4, [9.8, 1.0, -2.0, 2.0]), (5, [3.0, 0.5, -1.0, 0.25, 1.0, 2.0, -0.5])]
        cases += [(10 * f, [2.5]) for f in range(1, nf + 1)]
        for ltype, par in cases:
            out["t%d/dload_element_%d" % (et, ltype)] = ctx.dload_element(et, ltype, X, np.array(list(par) + [0.0] * (7 - len(par))), rho=7.8)

    for name in list(TG.TYPES) + ["mixed"]:
        m, groups = TD._mesh(name)
        dl = TD._list(m, groups, name)
        disp = 0.02 * np.cos(np.arange(3 * m.n_node) * 0.61)
        record("dload_%s" % name, lambda: {"load~atomic": ctx.dload_groups(m.coord, groups, TD.RHO, dl, factor=0.5)[0],
                                           "load_displaced~atomic": ctx.dload_groups(m.coord, groups, TD.RHO, dl, factor=0.5, disp=disp)[0]})

    # ---- refusals, and what the other entry points make of the same mesh
    def nothing(call):
        """call() for its refusal; accepted, it records nothing"""
        def run():
            call()
            return {}
        return run

    heat_call = lambda *a, **kw: nothing(RO._heat(hip, ctx, *a, **kw))
    col, bad = RO._collapsed(RO.HEXES), RO.HEXES[1:].copy()
    bad[0, 2] = RO.N + 1
    record("refuse/heat_collapsed_361", heat_call([(361, col)]))
    record("refuse/heat_unknown_type_ndof3", heat_call([(999, RO.HEXES)], ndof=3))
    record("refuse/heat_ndof3_empty_mesh", heat_call([(361, RO.HEXES)], ndof=3, coord=np.zeros((0, 3))))
    two = [(341, RO.TETS), (361, RO.HEXES[1:])]
    record("refuse/heat_duplicate_then_bad_node", heat_call([(341, RO._collapsed(RO.TETS)), (361, bad)], profile_groups=two))
    record("refuse/assemble_duplicate_then_bad_node", nothing(lambda: ctx.assemble_groups(RO.COORD, [(341, RO._collapsed(RO.TETS)), (361, bad)], E0, NU0)))
    for kind in ("dflux", "film", "radiate"):
        tail = (1.0,) if kind == "dflux" else (1.0, 300.0)
        for tag, (g, e, f) in (("group", (1, 5, 9)), ("element", (0, 5, 9)), ("face", (0, 1, 9))):
            record("refuse/heat_%s_%s" % (kind, tag), heat_call([(361, RO.HEXES)], **{kind: (RO.I0 + g, RO.I0 + e, RO.I0 + f) + tail}))
    for tag, (g, e, lt) in (("group", (1, 5, 90)), ("element", (0, 5, 90)), ("face", (0, 1, 90))):
        record("refuse/dload_%s" % tag, nothing(lambda: ctx.dload_groups(RO.COORD, [(361, RO.HEXES)], None, (RO.I0 + g, RO.I0 + e, RO.I0 + lt, np.zeros((1, 7))))))
    press = (RO.I0, RO.I0, RO.I0 + 10, np.array([[2.0, 0, 0, 0, 0, 0, 0]]))
    record("accept/dload_collapsed_361", lambda: {"load~atomic": ctx.dload_groups(RO.COORD, [(361, col)], None, press)[0]})
    ctx.close()

    def assemble_collapsed():
        hm = hip.hecmwST_local_mesh(n_node=RO.N)
        mat = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), [(361, col, 1, None)])
        c = hip.SolverContext()
        c.upload(mat, what=hip.FX_UP_PROFILE)
        c.assemble_groups(RO.COORD, [(361, col, 1, None)], E0, NU0)
        c.download_matrix(mat)
        c.close()
        return {k: getattr(mat, k) for k in ("D", "AL", "AU")}
    record("accept/assemble_collapsed_361", assemble_collapsed)

    # ---- fx_nl_get_load: the resident load vector with a list that follows the displacement and one that does not
    from frontistr_amd.mesh import CubeMesh
    m = CubeMesh(3)
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem, hm.elem_node_item = 8, m.conn.ravel()
    c = hip.SolverContext()
    c.upload(hip.hecmw_mat_con(hm, hip.hecmwST_matrix()), what=hip.FX_UP_PROFILE)
    solid = fstr.fstr_solid(c, m.coord, m.conn, fstr.tMaterial(1000.0, 0.3, nlgeom_flag=fstr.TOTALLAG))
    dl = fstr.tDload()
    for g, e, f in fstr.dload_faces(m.coord, [(361, m.conn)], m.coord[:, 2] == 3.0):
        dl.pressure(g, [e], f, 2.0)
    dl.gravity(0, np.arange(m.conn.shape[0]), 9.8, (0.2, 0.0, -1.0))
    cload = np.ascontiguousarray(np.sin(np.arange(3 * m.n_node) * 0.23))
    solid.set_state({"unode": 0.05 * np.cos(np.arange(3 * m.n_node) * 0.41)})
    for follow in (True, False):
        solid.set_dload(dl, 0.4, follow=follow)
        solid.set_dload_factor(0.7)
        hip._chk(hip.lib().fx_nl_begin_substep(c.h, hip._ptr(cload)))
        out["nl_get_load/follow%d~atomic" % follow] = solid.get_load()
    c.close()
    np.savez(path, **out)
    print("%d arrays of %d cases written to %s (library %s)" % (len(out), len({k.rsplit("/", 1)[0] for k in out}), path, hip.LIBPATH))
    return 0


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--compare":
        sys.exit(compare(args[1], args[2]))
    if len(args) == 2 and args[0] == "--dump":
        sys.exit(dump(args[1]))
    if len(args) == 2 and args[0] == "--dump-linear":
        sys.exit(dump_linear(args[1]))
    if len(args) == 2 and args[0] == "--dump-fields":
        sys.exit(dump_fields(args[1]))
    sys.exit(__doc__)
