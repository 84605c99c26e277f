"""The material point of the device nonlinear loop ON its branch edges (csrc/fx_nl_point.h, csrc/fx_yield.h as every element kernel
family inlines them) against the restatement tests/point_ref.py / tests/yield_ref.py.

The mechanism: under UPDATELAG with unode = dunode = 0 the displacement gradient is zero, every update kernel computes
trial = stress_bak bit for bit, and fstr_solid.set_state sets stress_bak / plstrain / istat / fstat per quadrature point.  One
element_update() therefore runs the return mapping of every point on a trial stress and a history chosen to the bit: exact ties of
principal stresses, a plastic strain exactly on a breakpoint of the hardening table, |f| on either side of tol, the `dlambda < 0`
reset, five iterations exhausted, the apex.  tests/test_point_ref.py asserts on the CPU that every case takes the branch it is built
for, in float64 and long double with outputs equal to 1e-12, and that a point function with a wrong select, comparison or iteration
count moves some case by more than 1e-9.

(a) the update of the six element types, six materials as sections of one context (groups 2 and 6 of the kernels);
(b) the tangents of hand-set states on the six types under UPDATELAG and on 361 B-bar / F-bar under INFINITE and TOTALLAG;
(c) the cases that keep their branch under a rounded trial stress, through the INFINITE / TOTALLAG updates of 361 B-bar, 361 F-bar,
    342 and 352 (the exact mechanism exists only under UPDATELAG, which F-bar refuses).

Tolerance: the project's nonlinear 1e-11 of the largest entry of the compared array; istat exactly; what an exit must not write,
bitwise."""
import functools

import numpy as np
import pytest

import fbar_ref as FB
import hyper_ref as H
import point_ref as P
import yield_ref as Y

pytestmark = pytest.mark.gpu
ETYPES = [361, 341, 342, 351, 352, 362]
TOL = 1e-11
BBAR, FBAR = 2, 4
NAMES = P.MATERIAL_NAMES


def _fmat(mat):
    from frontistr_amd import fstr
    if Y.is_yield(mat):
        fm = fstr.tMaterial(mat.E, mat.nu, plastic=True, harden=0, plconst=mat.plconst, nlgeom_flag=mat.nlgeom)
        fm.kind, fm.plconst4 = (fstr.MOHRCOULOMB if mat.kind == Y.MOHR else fstr.DRUCKERPRAGER), mat.plconst4
        return fm
    return fstr.tMaterial(mat.E, mat.nu, plastic=mat.plastic, harden=mat.harden, plconst=mat.plconst, table=mat.table if mat.harden == 1 else None,
                          nlgeom_flag=mat.nlgeom)


def _solid(hip, etype, m, mats, em, elemopt=BBAR):
    from frontistr_amd import fstr
    hm = hip.hecmwST_local_mesh(n_node=m.n_node)
    hm.nn_elem = m.conn.shape[1]
    hm.elem_node_item = m.conn.ravel()
    hecMAT = hip.hecmw_mat_con(hm, hip.hecmwST_matrix())
    ctx = hip.SolverContext()
    ctx.upload(hecMAT, what=hip.FX_UP_PROFILE)
    return ctx, fstr.fstr_solid(ctx, m.coord, m.conn, [_fmat(x) for x in mats], elem_mat=em, etype=etype, elemopt=elemopt)


def _close(a, b, tag, scale=None, tol=TOL):
    b = np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300) if scale is None else scale
    err = np.abs(np.asarray(a).reshape(b.shape) - b).max() / scale
    print("%s: %.3e (bound %.1e)" % (tag, err, tol))
    assert err < tol, "%s: %.3e" % (tag, err)


def _model(etype, m, mats, em, elemopt=BBAR):
    return FB.Model(m.coord, m.conn, mats, em) if elemopt == FBAR else Y.Model(etype, m.coord, m.conn, mats, em)


# ---- (a) exact trial stresses through the UPDATELAG update kernels ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _update_inputs(etype):
    """Mesh, sections, the case of every point, the state that puts it there, and what the restatement makes of it (computed once)"""
    nq = H.POINTS[etype]
    cases = [[c for c in P.CASES[k] if not c.apex] for k in NAMES]
    counts = [len(c) for c in cases]
    m, em = P.edge_mesh(etype, counts, nq)
    idx = P.deal(em, nq, counts)
    st = dict(stress_bak=np.zeros((m.n_elem, nq, 6)), plstrain=np.zeros((m.n_elem, nq)), fstat=np.zeros((m.n_elem, nq)),
              istat=np.zeros((m.n_elem, nq), dtype=np.int32))
    want = dict(stress=np.zeros((m.n_elem, nq, 6)), fstat=np.zeros((m.n_elem, nq)), istat=np.zeros((m.n_elem, nq), dtype=np.int32))
    keeps = np.zeros((m.n_elem, nq), dtype=bool)           # the exits that write nothing
    for e in range(m.n_elem):
        for q in range(nq):
            c = cases[em[e] - 1][idx[e, q]]
            st["stress_bak"][e, q], st["plstrain"][e, q], st["istat"][e, q], st["fstat"][e, q] = c.stress, c.plstrain, c.istat, c.fstat
            want["stress"][e, q], want["istat"][e, q], want["fstat"][e, q], _ = P.result(c)
            keeps[e, q] = c.exit in ("band", "elastic")
    for k, n in enumerate(counts):
        seen = np.bincount(idx[em == k + 1].ravel(), minlength=n)
        assert seen.min() >= 2, "%d %s: case %d lands on %d points" % (etype, NAMES[k], seen.argmin(), seen.min())
    return m, em, st, want, keeps


def _set_update_state(solid, m, st):
    z6 = np.zeros_like(st["stress_bak"])
    solid.set_state(dict(unode=np.zeros(3 * m.n_node), dunode=np.zeros(3 * m.n_node), stress=z6, strain=z6, strain_bak=z6, **st), latch=0)


@pytest.mark.parametrize("etype", ETYPES)
def test_update_on_the_branch_edges(hip, etype):
    m, em, st, want, keeps = _update_inputs(etype)
    if etype == 361:
        assert any(len(set(c)) < 8 for c in m.conn.tolist()), "no collapsed hexahedron in the 361 mesh"
    mats = [P.material(k) for k in NAMES]
    assert all(x.nlgeom == P.UPDATELAG for x in mats)
    ref = _model(etype, m, mats, em)
    for k, v in st.items():
        ref.st[k][:] = v
    rqf = ref.element_update()
    # the element routines handed every point its case: they return what the point function alone returns
    assert np.array_equal(ref.st["istat"], want["istat"])
    _close(ref.st["stress"], want["stress"], "%d restated update vs the point function alone, stress" % etype, tol=1e-12)
    _close(ref.st["fstat"], want["fstat"], "%d restated update vs the point function alone, fstat" % etype, tol=1e-12)
    ctx, solid = _solid(hip, etype, m, mats, em)
    _set_update_state(solid, m, st)
    qf = solid.element_update()
    s = solid.get_state()
    assert s["latch"] == 1 and ref.latch == 1
    assert np.array_equal(s["istat"], want["istat"]), "istat: %s" % (np.argwhere(s["istat"] != want["istat"])[:5].tolist(),)
    assert np.array_equal(s["stress_bak"], st["stress_bak"]) and not s["strain"].any()
    for k, name in enumerate(NAMES):
        sec = em == k + 1
        _close(s["stress"][sec], want["stress"][sec], "%d %s stress" % (etype, name))
        wrote = ~keeps[sec]
        _close(s["fstat"][sec][wrote], want["fstat"][sec][wrote], "%d %s fstat" % (etype, name))
    # band and elastic exits: the stress is the trial one, fstat what it held, to the bit
    assert keeps.sum() >= 2 * 10
    assert np.array_equal(s["stress"][keeps], st["stress_bak"][keeps]), "an early exit changed the stress"
    assert np.array_equal(s["fstat"][keeps], np.full(keeps.sum(), P.SENTINEL)), "an early exit wrote fstat"
    _close(qf, rqf, "%d element internal force" % etype)
    ctx.close()


@pytest.mark.parametrize("etype", ETYPES)
def test_zero_increment_hands_over_stress_bak(hip, etype):
    """The mechanism on the device: with a cohesion / yield stress no point reaches, the stress after the update is stress_bak"""
    m, em, st, _, _ = _update_inputs(etype)
    ctx, solid = _solid(hip, etype, m, [P.out_of_reach(k) for k in NAMES], em)
    _set_update_state(solid, m, st)
    solid.element_update()
    s = solid.get_state()
    assert not s["istat"].any()
    assert np.array_equal(s["stress"], st["stress_bak"]), "trial stress differs from stress_bak"
    assert np.array_equal(s["fstat"], st["fstat"])
    ctx.close()


@pytest.mark.parametrize("etype", ETYPES)
def test_apex_does_not_stop_the_update(hip, etype):
    """Hydrostatic tension beyond the apex: J2 = 0, the reference computes NaN (Mohr-Coulomb) or divides by sqrt(J2) = 0
    (Drucker-Prager) and goes on.  So do the kernels: non-finite numbers in the same positions, no error; the context then serves a
    sound update."""
    nq = H.POINTS[etype]
    m = H.gpu_mesh(etype)
    names = ("mohr", "drucker")
    mats = [P.material(k) for k in names]
    apex = [next(c for c in P.CASES[k] if c.apex) for k in names]
    calm = [next(c for c in P.CASES[k] if c.name == "unloading") for k in names]      # (a zero stress has J2 = 0 as well)
    em = (1 + np.arange(m.n_elem) % 2).astype(np.int32)
    hit = np.zeros((m.n_elem, nq), dtype=bool)
    hit.ravel()[::3] = True
    ref = _model(etype, m, mats, em)
    for e in range(m.n_elem):
        ref.st["stress_bak"][e, hit[e]] = apex[em[e] - 1].stress
        ref.st["stress_bak"][e, ~hit[e]] = calm[em[e] - 1].stress
    st = {k: ref.st[k].copy() for k in ("stress_bak", "plstrain", "fstat", "istat")}
    with np.errstate(all="ignore"):
        ref.element_update()
    ctx, solid = _solid(hip, etype, m, mats, em)
    _set_update_state(solid, m, st)
    solid.element_update()                               # no error word: the reference does not stop here
    s = solid.get_state()
    assert s["latch"] == 1 and np.array_equal(s["istat"], ref.st["istat"]) and np.array_equal(s["istat"] != 0, hit)
    for key in ("stress", "fstat"):
        fin = np.isfinite(ref.st[key])
        assert np.array_equal(np.isfinite(s[key]), fin), key
        _close(s[key][fin], ref.st[key][fin], "%d apex, finite part of %s" % (etype, key), max(np.abs(ref.st[key][fin]).max(), 1e-300))
    assert not np.isfinite(s["stress"][hit]).any() and np.isfinite(s["fstat"][hit & (em == 2)[:, None]]).all()
    # a sound update afterwards
    u = np.zeros_like(m.coord)
    u[:, 0] = 0.05 * m.coord[:, 0] + 0.04 * m.coord[:, 1] + 0.02 * m.coord[:, 2]
    ref = _model(etype, m, mats, em)
    ref.dunode[:] = u.ravel()
    z = {k: np.zeros_like(v) for k, v in st.items()}
    _set_update_state(solid, m, z)
    solid.set_state(dict(dunode=u.ravel()), latch=0)
    qf, rqf = solid.element_update(), ref.element_update()
    s = solid.get_state()
    assert np.array_equal(s["istat"], ref.st["istat"]) and ref.st["istat"].any()
    _close(s["stress"], ref.st["stress"], "%d stress after the apex" % etype)
    _close(qf, rqf, "%d element internal force after the apex" % etype)
    ctx.close()


# ---- (b) tangents at hand-set states ---------------------------------------------------------------------------------------------------------
TANGENT_RUNS = [(et, P.UPDATELAG, BBAR) for et in ETYPES] + [(361, g, o) for o in (BBAR, FBAR) for g in (P.INFINITE, P.TOTALLAG)]


@functools.lru_cache(maxsize=None)
def _tangent_inputs(etype):
    nq = H.POINTS[etype]
    states = P.tangent_states()
    counts = [len(states[k]) for k in NAMES]
    m, em = P.edge_mesh(etype, counts, nq)
    idx = P.deal(em, nq, counts)
    st = dict(stress=np.zeros((m.n_elem, nq, 6)), fstat=np.zeros((m.n_elem, nq)), istat=np.zeros((m.n_elem, nq), dtype=np.int32))
    for e in range(m.n_elem):
        for q in range(nq):
            x = states[NAMES[em[e] - 1]][idx[e, q]]
            st["stress"][e, q], st["istat"][e, q], st["fstat"][e, q] = x.stress, x.istat, x.fstat
    for k, n in enumerate(counts):
        assert np.bincount(idx[em == k + 1].ravel(), minlength=n).min() >= 2
    return m, em, st


@pytest.mark.parametrize("etype,nlgeom,elemopt", TANGENT_RUNS,
                         ids=["%d-%s-%s" % (et, ("infinite", "totallag", "updatelag")[g], "fbar" if o == FBAR else "std") for et, g, o in TANGENT_RUNS])
def test_tangents_of_hand_set_states(hip, etype, nlgeom, elemopt):
    """The tangent reads the stored stress / istat / fstat whatever the flag: the returned states of the plastic cases, sin 3 theta = +-1
    (C1 = 0, C2 = sqrt 3, C3 = 0), plastic strains on the edges of the hardening table (H = 0 outside it) and laws"""
    m, em, st = _tangent_inputs(etype)
    mats = [P.material(k, nlgeom) for k in NAMES]
    for name, states in P.tangent_states().items():          # the hand-set edge states take the edge branch
        for x in states:
            if x.branch is not None:
                info = {}
                P.tangent(P.material(name, nlgeom), x.stress, x.istat, np.float64(x.fstat), info)
                assert info["branch"] == x.branch, (name, x.name, info)
    ref = _model(etype, m, mats, em, elemopt)
    for k, v in st.items():
        ref.st[k][:] = v
    want = ref.element_tangents()
    elastic = _model(etype, m, mats, em, elemopt)
    elastic.st["stress"][:] = st["stress"]
    assert np.abs(want - elastic.element_tangents()).max() > 1e-3 * np.abs(want).max(), "the plastic states do not change the tangent"
    ctx, solid = _solid(hip, etype, m, mats, em, elemopt)
    z6 = np.zeros_like(st["stress"])
    solid.set_state(dict(unode=np.zeros(3 * m.n_node), dunode=np.zeros(3 * m.n_node), strain=z6, stress_bak=z6, strain_bak=z6,
                         plstrain=np.zeros_like(st["fstat"]), **st), latch=0)
    ke = solid.element_tangents()
    for k, name in enumerate(NAMES):
        _close(ke[em == k + 1], want[em == k + 1], "%d nlgeom %d elemopt %d %s tangent" % (etype, nlgeom, elemopt, name))
    ctx.close()


# ---- (c) the cases with a margin through INFINITE, TOTALLAG and F-bar updates -----------------------------------------------------------------
@pytest.mark.parametrize("etype,nlgeom,elemopt", P.AFFINE_RUNS,
                         ids=["%d-%s-%s" % (et, ("infinite", "totallag")[g], "fbar" if o == FBAR else "std") for et, g, o in P.AFFINE_RUNS])
def test_branches_through_the_other_flags(hip, etype, nlgeom, elemopt):
    """Disconnected unit cells, one per case, under the affine displacement whose strain is D^-1 . trial (point_ref.affine_model): the
    Drucker-Prager reset, the exhausted RAMBERG-OSGOOD return, the six Mohr-Coulomb orderings, the return that crosses a breakpoint of
    the table, unloading from istat = 1 -- groups 0, 1, 4, 5 of the B-bar, STF_C3 and F-bar update kernels"""
    P.check_affine(etype, nlgeom, elemopt)               # every point in the branch of its case, with the margins
    m, em, per_elem, st, ref = P.affine_model(etype, nlgeom, elemopt)
    dunode = ref.dunode.copy()
    rqf = ref.element_update()
    ctx, solid = _solid(hip, etype, m, [P.material(k, nlgeom) for k in P.AFFINE_NAMES], em, elemopt)
    z6 = np.zeros_like(ref.st["stress"])
    solid.set_state(dict(unode=np.zeros_like(dunode), dunode=dunode, stress=z6, strain=z6, stress_bak=z6, strain_bak=z6, **st), latch=0)
    qf = solid.element_update()
    s = solid.get_state()
    tag = "%d nlgeom %d elemopt %d " % (etype, nlgeom, elemopt)
    assert s["latch"] == 1 and np.array_equal(s["istat"], ref.st["istat"]), tag + "istat"
    keeps = np.array([c.exit == "elastic" for c in per_elem])
    assert keeps.any() and np.array_equal(s["fstat"][keeps], np.full((keeps.sum(), s["fstat"].shape[1]), P.SENTINEL)), "unloading wrote fstat"
    for k, name in enumerate(P.AFFINE_NAMES):
        sec = em == k + 1
        _close(s["stress"][sec], ref.st["stress"][sec], tag + name + " stress")
        wrote = sec & ~keeps
        if wrote.any():
            _close(s["fstat"][wrote], ref.st["fstat"][wrote], tag + name + " fstat")
    _close(s["strain"], ref.st["strain"], tag + "strain")
    _close(qf, rqf, tag + "element internal force")
    ctx.close()
