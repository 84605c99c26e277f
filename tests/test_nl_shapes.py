"""The cases of tests/nl_shapes.py reach what they are there for (CPU; nothing here touches a GPU).

For every (family, group) the host instantiates, the launch restatement of nl_shapes must show, in some case, for the tangent and for
the update kernel: a one-launch-per-group launch of at least two workgroups whose last one is partly filled; a workgroup with every
slot filled; a coloured-scatter launch that starts behind the head of the list (e0 != 0), has at least two workgroups and a partly
filled last one; the list walked through colors.order and the list walked in element order.  A group without a case fails here with
the (family, group, condition) it lacks.

The conditions under which the 1e-11 bound of tests/test_gpu_nl_shapes.py means something are asserted for the new inputs with the
checks of test_hyper_ref.py, test_visco_ref.py, test_yield_ref.py, test_point_ref.py (the Mises point), test_fbar_ref.py,
test_nl_thermal_ref.py and test_c3_nl_ref.py: float64 against long double of the restatement at every point, strains that strain the
material, every dt / tau a factor of ten from hvisc's switch, the creep iteration far below its cap and a creep strain that counts,
every elastoplastic point 10 tol from the edges of its return mapping with points on both sides, the single-precision share."""
import numpy as np
import pytest

import hyper_ref as H
import nl_shapes as S
import test_visco_ref as TV
import visco_ref as V

FACTS = S.kernel_facts()
CONDITIONS = ("tangent: two workgroups, last partly filled", "tangent: a full workgroup", "tangent: coloured launch behind the head of the list",
              "update: two workgroups, last partly filled", "update: a full workgroup", "update: walked through colors.order",
              "update: walked in element order")
_LAUNCHES = {}


def _launches(cid):
    if cid not in _LAUNCHES:
        _LAUNCHES[cid] = S.case_launches(S.CASES[cid], FACTS)
    return _LAUNCHES[cid]


def reached(cases):
    """{(family, group, TH): set of CONDITIONS some case of `cases` gives}"""
    out = {}
    for cid in cases:
        case = S.CASES[cid]
        tep, uep = FACTS["epb"][case.fam]
        per_group, lists = _launches(cid)
        # nl_launch_stiffness takes the TH = 1 tangent kernels only with an elastic table in the context (the update kernels whenever
        # thermal strain is on): a thermal case without one counts for the update alone
        tangent = not case.th or any(getattr(x, "elastic_table", None) is not None for x in case.materials())
        for g, L in per_group.items():
            got = out.setdefault((case.fam, g, case.th), set())
            for x in L["out"] if tangent else []:
                if x["what"] == "out" and x["workgroups"] >= 2 and (x["last"] < tep or tep == 1):
                    got.add(CONDITIONS[0])
            if tangent and any(x["e1"] - x["e0"] >= x["epb"] for x in L["out"] + L["scatter"] if x["what"] != "add"):
                got.add(CONDITIONS[1])
            for x in L["scatter"] if tangent else []:
                if case.scatter and x["what"] == "colour" and x["e0"] != 0 and x["workgroups"] >= 2 and (x["last"] < tep or tep == 1):
                    got.add(CONDITIONS[2])
            for x in L["update"]:
                if x["what"] == "update" and x["workgroups"] >= 2 and x["last"] < uep:
                    got.add(CONDITIONS[3])
                if x["e1"] - x["e0"] >= uep:
                    got.add(CONDITIONS[4])
                if x["what"] == "update":
                    got.add(CONDITIONS[5] if x["walk"] == "order" else CONDITIONS[6])
    return out


def missing(cases):
    got = reached(cases)
    return ["%s group %d%s: %s" % (fam, g, " TH = 1" if th else "", c) for fam, g, th in S.instantiated(FACTS)
            for c in CONDITIONS if c not in got.get((fam, g, th), ())]


def test_kernel_table_is_read_from_the_sources():
    assert FACTS["n_groups"] >= 10
    assert [FACTS["flag"](g) for g in range(10)] == [0, 1, 2, 1, 0, 1, 2, 0, 1, 2]
    assert [g for g in range(FACTS["n_groups"]) if not FACTS["fbar"](g)] == [g for g in range(FACTS["n_groups"]) if FACTS["flag"](g) == 2]
    assert [g for g in range(10) if not FACTS["thermal"](g)] == [7, 8, 9]
    # the table of the kernels' own comments: 361 32 / 32, F-bar 8 / 32, 341 4 waves x 6 / 256, 342 4 / 64, 351 4 waves x 3 / 32
    assert FACTS["epb"] == {"361": (32, 32), "361f": (8, 32), "341": (24, 256), "342": (4, 64), "351": (12, 32), "352": (2, 8), "362": (1, 2)}
    import nl_thermal_ref as NT
    for fam in S.FAMILIES:
        assert FACTS["epb"][fam][1] == NT.update_elems_per_workgroup(fam)


def test_every_instantiated_kernel_has_a_case():
    covered = {(S.CASES[c].fam, g, S.CASES[c].th) for c in S.CASES for g in _launches(c)[0]}
    inst = set(S.instantiated(FACTS))
    assert covered == inst, "no case: %s; not instantiated: %s" % (sorted(inst - covered), sorted(covered - inst))


def test_every_group_reaches_every_condition():
    lack = missing(list(S.CASES))
    assert not lack, "\n".join(lack)


def test_removing_a_case_is_noticed():
    """the guard guards: without the one-material NORTON case of 341 the update of group 9 has no second workgroup any more"""
    lack = missing([c for c in S.CASES if c != "341_solo_norton"])
    assert any(x.startswith("341 group 9: update: two workgroups") for x in lack), lack


def test_launch_restatement_on_a_hand_counted_mesh():
    """hyper_ref.gpu_mesh(361): 8 hexahedra of 8 colours and one collapsed one; two groups dealt in turn"""
    m = H.gpu_mesh(361)
    eg = np.array([1, 3] * 4 + [3])
    lists = S.part_lists(m.conn, m.n_node, eg, 10)
    assert not lists["atomic"] and sorted(lists["order"]) == list(range(8)) and lists["dup"] == [8]
    assert lists["order"][:4] == [0, 2, 4, 6] and lists["order"][4:] == [1, 3, 5, 7]
    assert lists["dup_off"][1] == [] and lists["dup_off"][3][0] == 0 and lists["dup_off"][3][-1] == 1
    t = S.tangent_launches(lists, 3, 32, False)
    assert [x["what"] for x in t] == ["colour"] * 4 + ["dup", "add"]
    assert [(x["e0"], x["e1"]) for x in t[:4]] == [(4, 5), (5, 6), (6, 7), (7, 8)]
    t = S.tangent_launches(lists, 3, 32, True)
    assert [(x["what"], x["e0"], x["e1"], x["workgroups"], x["last"]) for x in t] == [("out", 4, 8, 1, 4), ("dup", 0, 1, 1, 1)]
    u = S.update_launches(lists, 1, 32)
    assert [(x["what"], x["walk"], x["e0"], x["e1"]) for x in u] == [("update", "order", 0, 4)]
    forced = S.part_lists(m.conn, m.n_node, eg, 10, force_atomic=True)
    assert forced["atomic"] and forced["dup"] == [] and forced["order"] == [0, 2, 4, 6, 1, 3, 5, 7, 8]
    one = S.part_lists(m.conn[:8], m.n_node, np.full(8, 3), 10)
    assert S.update_launches(one, 3, 32)[0]["walk"] == "elements"


def test_pies_and_the_renumbered_cube():
    from frontistr_amd.mesh import color_elements
    # PieMesh(24, 2, 2): 48 of 96 elements collapsed; at least two groups hold collapsed elements in at least two colours
    for cid in ("361_pie24", "361f_pie24", "361_pie24_creep"):
        case = S.CASES[cid]
        m = S.mesh_of(case.mesh)
        twice = np.array([len(set(c)) < 8 for c in m.conn.tolist()])
        assert m.n_elem == 96 and twice.sum() == 48
        per_group, lists = _launches(cid)
        assert not lists["atomic"] and len(lists["dup"]) == 48
        several = 0
        for g in per_group:
            doff = lists["dup_off"][g]
            colours = sum(1 for a, b in zip(doff[:-1], doff[1:]) if b > a)
            print(cid, "group", g, "collapsed elements per colour", [b - a for a, b in zip(doff[:-1], doff[1:]) if b > a])
            several += colours >= 2
            assert [x["what"] for x in per_group[g]["scatter"]].count("add") == colours
        assert several >= 2 and len(per_group) == 3
    # PieMesh(33, 1, 2): the axis nodes are in 66 elements, the colouring fails -- the atomic fallback with no variable set
    m = S.mesh_of("pie33")
    assert color_elements(m.conn, m.n_node) is None
    per_group, lists = _launches("361_pie33")
    assert lists["atomic"] and not lists["dup"] and len(per_group) == 3
    assert all([x["what"] for x in L["scatter"]] == ["atomic"] for L in per_group.values())
    # renumber(CubeMesh(7), 11): many small colours, two sections
    m = S.mesh_of("renum7")
    col = color_elements(m.conn, m.n_node)
    counts = np.bincount(col)
    print("renumbered cube: %d colours of %d .. %d" % (counts.size, counts.min(), counts.max()))
    assert counts.size >= 12
    per_group, lists = _launches("361_renum7")
    assert len(per_group) == 2 and all(len([x for x in L["scatter"] if x["what"] == "colour"]) >= 12 for L in per_group.values())


def test_one_forced_atomic_case_per_family():
    assert sorted(S.CASES[c].fam for c in S.CASES if S.CASES[c].atomic_child) == sorted(S.FAMILIES)


# ---- the inputs determine the restated numbers -----------------------------------------------------------------------------------------
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].helper == "hyper"])
def test_hyperelastic_inputs_are_well_conditioned(cid):
    """test_hyper_ref.test_gpu_inputs_are_well_conditioned on the strains this case stores at its hyperelastic points (none left out),
    and on the zero strain of the first tangent; an ELASTIC section is linear in its strain: nothing to condition"""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    m, ref = S.CASES[cid].build()
    hyper = [e for e in range(ref.conn.shape[0]) if H.kind_of(ref.mat(e)) in (H.MOONEY, H.ARRUDA)]
    ref.element_update()
    assert np.abs(ref.st["strain"]).max() > 0.02, "the inputs do not strain the material"
    if not hyper:
        return
    mat = ref.mat(hyper[0])
    strains = np.concatenate([ref.st["strain"][hyper].reshape(-1, 6), np.zeros((1, 6))])
    smax = max(np.abs(H.stress_update(mat, e)).max() for e in strains)
    worst_s = worst_d = 0.0
    for e in strains:
        el = e.astype(np.longdouble)
        S64, D64, Sl, Dl = H.stress_update(mat, e), H.tangent(mat, e), H.stress_update(mat, el), H.tangent(mat, el)
        worst_s = max(worst_s, float(np.abs(S64 - Sl).max()) / smax)
        worst_d = max(worst_d, float(np.abs(D64 - Dl).max() / np.abs(Dl).max()))
    print("%s: %d points, |E| to %.3f, float64 vs long double: stress %.2e, tangent %.2e"
          % (cid, len(strains), np.abs(strains).max(), worst_s, worst_d))
    assert np.abs(strains).max() > 0.02
    assert worst_s <= 1e-12 and worst_d <= 1e-12


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].helper in ("visco", "creep")])
def test_viscoelastic_and_creep_inputs_are_well_conditioned(cid):
    """test_visco_ref's check of every viscoelastic and NORTON point in both of the stress updates a comparison makes"""
    case = S.CASES[cid]
    m, ref = case.build()
    if not any(V.is_visco(x) or V.is_creep(x) for x in ref.mats):
        return
    TV.check_conditioning(cid, [ref], case.amplitude())


@pytest.mark.parametrize("cid", [c for c in S.CASES if "el_ul" in S.CASES[c].mats and S.CASES[c].etype != 361])
def test_updated_lagrange_single_precision_share(cid):
    """test_c3_nl_ref's check on the new inputs: the share of stress components that two orders of summation put on different
    single-precision neighbours stays below the 1 % the two-tier rule of the GPU comparison allows.  On the ELASTIC UPDATELAG
    elements of every case that has them: tet_nl_ref / c3_nl_ref are the restatements that take an order of summation."""
    import c3_nl_ref as N
    import c3_ref as R
    import tet_nl_ref as TN
    case = S.CASES[cid]
    m, ref = case.build()
    Model = TN.Model if case.etype in (341, 342) else N.Model
    el = [e for e in range(ref.conn.shape[0]) if ref.mat(e) is ref.mats[case.mats.index("el_ul")]]
    assert el
    res = []
    for order in (None, list(range(R.NN[case.etype]))[::-1]):
        mod = Model(case.etype, m.coord, m.conn[el], ref.mats[case.mats.index("el_ul")])
        mod.st = {k: v[el].copy() for k, v in ref.st.items()}
        mod.unode[:], mod.dunode[:] = ref.unode, ref.dunode
        mod.element_update(order)
        res.append((mod.st["stress"].copy(), mod.dstress.copy()))
    scale = np.abs(res[0][1]).max()
    diff = np.abs(res[0][0] - res[1][0]) / scale
    share = (diff > 1.0e-11).mean()
    print("%s: %.4f of the components differ by more than 1e-11, max %.3e (2 ulp = %.3e)" % (cid, share, diff.max(), 2.0 * 2.0 ** -23))
    assert diff.max() <= 2.0 * 2.0 ** -23
    assert share <= 0.01


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].helper == "yield"])
def test_yield_inputs_meet_the_margins(cid):
    """test_yield_ref's margins and float64 / long double agreement at every Drucker-Prager point of the case, per section: no point
    within 10 tol of |f| = tol, none through the dlambda < 0 reset, a quarter of the points plastic and a tenth elastic"""
    import test_yield_ref as TY
    import yield_ref as Y
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    case = S.CASES[cid]
    m = S.mesh_of(case.mesh)
    em = case.elem_mat(m)
    seed, c = Y.SHAPE_CASES[case.yield_key]
    ne = m.conn.shape[0]
    mises = []
    for k, mat in enumerate(case.materials()):
        if not (Y.is_yield(mat) or mat.plastic):
            continue
        elems = np.arange(ne) if em is None else np.nonzero(em == k + 1)[0]
        family = "mises" if not Y.is_yield(mat) else ("mohr" if mat.kind == Y.MOHR else "drucker")
        if case.fam == "361f":
            import fbar_ref as FB
            trial = FB.trial_stresses(family, mat.nlgeom, seed, m)
        else:       # (the trial stress is the elastic one: the same for the three families on yield_ref's constants)
            trial = Y.trial_stresses(case.etype, "drucker", mat.nlgeom, seed, 1.0, m)
        trial = trial.reshape(ne, -1, 6)[elems].reshape(-1, 6)
        if family != "mises":
            TY.check_points(mat, trial, "%s section %d" % (cid, k + 1))
            continue
        # Mises: the edge of its return, both sides of it, and the point in float64 against long double (test_point_ref's condition)
        import point_ref
        mises.append(trial)
        f = Y.mises_f(trial, mat.plconst[0])
        print("%s section %d: %d Mises points, %.0f %% plastic, min ||f| - tol| %.3g" % (cid, k + 1, len(trial), 100 * (f > 0).mean(),
                                                                                        np.abs(np.abs(f) - Y.TOL).min()))
        worst = 0.0
        smax = np.abs(trial).max()
        for s in trial:
            a = point_ref.backward_euler(mat, s, 0.0, 0, 0.0)
            b = point_ref.backward_euler(mat, s.astype(np.longdouble), np.longdouble(0), 0, np.longdouble(0))
            assert a[1] == b[1] and b[0].dtype == np.longdouble
            worst = max(worst, float(np.abs(a[0] - b[0]).max()) / smax, abs(float(a[2]) - float(b[2])) * mat.E / smax)
        assert worst <= 1e-12, worst
    if mises:
        assert Y.mises_margins_hold(mises, case.materials()[0].plconst[0])


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].th])
def test_thermal_update_float64_against_longdouble(cid):
    """test_nl_thermal_ref.test_update_float64_against_longdouble on the new inputs: stress, strain and element forces of the restated
    update within 1e-12 of the largest entry.  As there, a case that runs UPDATE_C3's UPDATELAG branch is left to the single-precision
    rule: its rounding to default real can fall on either side in the two precisions."""
    import nl_thermal_ref as NT
    case = S.CASES[cid]
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    d = case.build()
    if any(NT.is_elastoplastic(x) for x in d["mats"]):
        import test_nl_thermal_ref as TT
        TT.check_plastic_points(d)
    if case.single_precision():
        return
    a, b = NT.model_of(d), NT.model_of(d).widen()
    qa, qb = a.element_update()[0], b.element_update()[0]
    assert qb.dtype == np.longdouble and b.parts[0]["st"]["stress"].dtype == np.longdouble
    for k in ("stress", "strain", "fstat"):
        x, y = a.parts[0]["st"][k], b.parts[0]["st"][k]
        assert np.abs(x - y).max() <= 1e-12 * max(np.abs(y).max(), 1e-3 if k == "fstat" else 1e-300), (cid, k)
    assert np.abs(qa - qb).max() <= 1e-12 * np.abs(qb).max()
    assert np.array_equal(a.parts[0]["st"]["istat"], b.parts[0]["st"]["istat"])
    assert a.parts[0]["st"]["istat"].any() == any(NT.is_elastoplastic(x) for x in d["mats"])
    tc = d["temperature"]
    assert tc.min() < NT.ELASTIC_TAB[0, 2] and tc.max() > NT.ELASTIC_TAB[-1, 2] and ((tc > 0.0) & (tc < 300.0)).any()


@pytest.mark.parametrize("cid", [c for c in S.CASES if S.CASES[c].fam == "361f" and not S.CASES[c].th])
def test_fbar_inputs_are_well_conditioned(cid):
    """test_fbar_ref's conditions on every F-bar case (the thermal ones: test_thermal_update_float64_against_longdouble): the F-bar
    element model in float64 against long double -- tangents before and after the update, stress, strain and internal force of the
    ELASTIC and hyperelastic sections; the trial stresses of the elastoplastic sections (test_plastic_gpu_inputs_keep_off_the_branch_edges;
    their margins: test_yield_inputs_meet_the_margins); stress and internal force of the viscoelastic sections -- to 1e-12 of the
    largest entry, no element left out."""
    import copy
    import fbar_ref as FB
    import test_fbar_ref as TF
    import yield_ref as Y
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    case = S.CASES[cid]
    m, ref = case.build()
    ref0 = copy.deepcopy(ref)
    got = dict(k0=ref.element_tangents())
    got["qf"] = ref.element_update()
    got.update(stress=ref.st["stress"], strain=ref.st["strain"], k1=ref.element_tangents())
    ld = np.longdouble
    coord, u, du = m.coord.astype(ld), ref0.unode.astype(ld).reshape(-1, 3), ref0.dunode.astype(ld).reshape(-1, 3)
    ne = m.conn.shape[0]
    kinds = np.array(["visco" if V.is_visco(ref.mat(e)) else ("plastic" if Y.is_yield(ref.mat(e)) or ref.mat(e).plastic else "elastic") for e in range(ne)])
    el = np.nonzero(kinds == "elastic")[0]
    if el.size:
        want = TF._longdouble_model(m, ref.mat, ref0.unode, ref0.dunode, el)
        TF.check_against_longdouble({k: v[el] for k, v in got.items()}, want, cid)
    pl = np.nonzero(kinds == "plastic")[0]
    if pl.size:
        z = np.zeros(8)
        seed = Y.SHAPE_CASES[case.yield_key][0]
        for flag in sorted({ref.mat(e).nlgeom for e in pl}):
            sec = [e for e in pl if ref.mat(e).nlgeom == flag]
            far = FB.gpu_material("drucker", flag, 1.0e12)
            trial = FB.trial_stresses("drucker", flag, seed, m).reshape(ne, 8, 6)[sec]
            wide = np.array([FB.update_c3d8fbar(coord[m.conn[e] - 1], u[m.conn[e] - 1], du[m.conn[e] - 1], far, z, z.astype(np.int32), z)[1] for e in sec])
            err = float(np.abs(trial - wide).max() / np.abs(wide).max())
            print("%s flag %d: %d elastoplastic elements, trial stress float64 vs long double %.2e" % (cid, flag, len(sec), err))
            assert wide.dtype == ld and err <= 1e-12
    vi = np.nonzero(kinds == "visco")[0]
    if vi.size:
        s64, q64 = got["stress"][vi], got["qf"][vi]
        worst = 0.0
        for k, e in enumerate(vi):
            nd, mat = m.conn[e] - 1, ref.mat(e)
            qf, s, _ = V.update_c3d8fbar(coord[nd], u[nd] + du[nd], mat, ref0.hist[e][:, :mat.width].astype(ld), ref0.tincr)
            worst = max(worst, float(np.abs(s - s64[k]).max() / np.abs(s64).max()), float(np.abs(qf - q64[k]).max() / np.abs(q64).max()))
        print("%s: %d viscoelastic elements, stress and internal force float64 vs long double %.2e" % (cid, vi.size, worst))
        assert worst <= 1e-12
