#!/usr/bin/env python3
"""Bitwise A/B of the nonlinear element kernels between two builds of libfistr_hip.so (a refactor must not move a bit).

    ab_nl_bitwise.py --dump OUT.npz [--lib PATH]     run the cases below in this process, write every output
    ab_nl_bitwise.py --compare A.npz B.npz           per array: equal bit for bit, or the first difference; exit 1 on any

Not a test: the second build (the parent commit's) is not in the repository.  Run --dump once with each library, each in a fresh
process (a few seconds), then --compare.

Cases, on the small distorted meshes of the GPU tests (hyper_ref.gpu_mesh: a handful of elements; 361 with a collapsed hexahedron):
  every type 361, 341, 342, 351, 352, 362 x group 0..6 -- ELASTIC and Mises for each NLGEOM flag, Mooney-Rivlin (group 3),
  Drucker-Prager and Mohr-Coulomb for each flag (yield_ref.gpu_case: points on both sides of the surface) --,
  a two-section context per type (Mises UPDATELAG beside ELASTIC TOTALLAG), and two fx_nl_init_groups contexts (hexahedra + wedges +
  tetrahedra, linear and quadratic) with the same two sections.
Outputs per case: element tangents before the first update and after it (the latch), the per-element internal forces of the update,
the state after the update and after fx_nl_commit, and D / AL / AU of the coloured scatter (fx_nl_stiffness_at, fx_download_matrix)
before and after the update.  Nodal QFORCE and the FX_ASM_ATOMIC scatter are sums of fp64 atomics in no fixed order: not compared."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STATE = ("stress", "strain", "stress_bak", "strain_bak", "plstrain", "fstat", "istat")
ETYPES = (361, 341, 342, 351, 352, 362)
E0, NU0 = 206900.0, 0.29


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
        bad.append(k)
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%-60s DIFFERS: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            continue
        xb, yb = x.ravel().view(np.uint8).reshape(x.size, -1), y.ravel().view(np.uint8).reshape(y.size, -1)
        i = int(np.flatnonzero((xb != yb).any(axis=1))[0])
        print("%-60s DIFFERS: %d of %d values, first at %d: %r against %r" % (k, int((xb != yb).any(axis=1).sum()), x.size, i,
                                                                              x.ravel()[i], y.ravel()[i]))
    print("%d arrays differ" % len(bad) if bad else "all arrays equal bit for bit")
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
            et, conn, _, em = groups[0]
            hm.nn_elem = conn.shape[1]
            hm.elem_node_item = conn.ravel()
            hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
        else:
            hecMAT = hip.hecmw_mat_con_groups(hm, hip.hecmwST_matrix(), groups)
        ctx = hip.SolverContext()
        ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
        fm = [fmat(x) for x in mats]
        if len(groups) == 1:
            solid = fstr.fstr_solid(ctx, mesh.coord, conn, fm if len(fm) > 1 else fm[0], elem_mat=em, etype=et)
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

    def single(name, etype, mesh, mats, em, unode=None, dunode=None, history=True):
        groups = [(etype, mesh.conn, 2, em)]
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
    np.savez(path, **out)
    print("%d arrays of %d cases written to %s (library %s)" % (len(out), len({k.split("/")[0] for k in out}), path, hip.LIBPATH))
    return 0


if __name__ == "__main__":
    from _libarg import take_lib
    take_lib()
    args = sys.argv[1:]
    if len(args) == 3 and args[0] == "--compare":
        sys.exit(compare(args[1], args[2]))
    if len(args) == 2 and args[0] == "--dump":
        sys.exit(dump(args[1]))
    sys.exit(__doc__)
