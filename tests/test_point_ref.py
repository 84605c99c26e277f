"""The edge cases of tests/point_ref.py mean what they claim: the condition under which tests/test_gpu_point_edges.py compares the
device's material point with the restatement ON the branch edges, at 1e-11.

(a) Every case takes the exit it was built for, with the iteration count, table rows, maxp / minp / mm it states, in float64 and in
    np.longdouble alike; the outputs of the two precisions agree to 1e-12 of the largest entry (the bound of test_yield_ref.py), no case
    exempt -- the apex cases as `non-finite in the same positions`.  An exact edge is no obstacle to that: a tie of two equal doubles,
    a plastic strain equal to a breakpoint, are the same comparison in every arithmetic.  Cases BESIDE an edge state their margin and
    it is asserted.
(b) The float64 numpy Mises point is the C oracle's: istat and exit exactly, values to 1e-12.
(c) The mechanism: with ddu = 0 under UPDATELAG the numpy update routines hand the point function a trial stress array_equal to
    stress_bak, on a distorted element of each of the six types.
(d) Coverage: the (family, exit) pairs and the (maxp, minp, mm) triples the table reaches are the ones written out here.
(e) Discrimination: each deliberately wrong point function (point_ref.MUTANTS) moves the restated output of at least one case by more
    than 1e-9 of its largest entry -- 100 times the GPU tolerance -- or changes its istat (update cases and tangent states).
"""
import numpy as np
import pytest

import c3_nl_ref as CN
import hyper_ref as H
import point_ref as P
import tet_nl_ref as T
import yield_ref as Y

EPS = np.finfo(np.float64).eps
WIDE = np.finfo(np.longdouble).eps < EPS
TYPES = [361, 341, 342, 351, 352, 362]
DTYPES = [np.float64, np.longdouble]
CASE_IDS = ["%s-%s" % (c.mat, c.name) for c in P.all_cases()]


def _run(case, dtype, **kw):
    info = {}
    s, ist, fs = case.run(dtype, info, **kw)
    return np.asarray(s), int(ist), fs, info


@pytest.mark.parametrize("case", P.all_cases(), ids=CASE_IDS)
def test_case_takes_its_branch(case):
    for dtype in DTYPES:
        s, ist, fs, info = _run(case, dtype)
        tag = (case.mat, case.name, dtype.__name__, info)
        assert s.dtype == dtype
        assert info["exit"] == case.exit, tag
        assert ist == {"band": 1, "elastic": 0, "reset": 0, "converged": 1, "exhausted": 1}[case.exit], tag
        if case.exit in ("band", "elastic"):
            assert np.array_equal(s, case.stress.astype(dtype)) and fs == P.SENTINEL and info["iterations"] == 0, tag
        else:
            assert case.apex or float(fs) != P.SENTINEL
        e = case.expect
        if "iterations" in e:
            assert info["iterations"] == e["iterations"], tag
        if "triple" in e:
            assert (info["maxp"], info["minp"], info["mm"]) == e["triple"], tag
        if "first" in e:
            assert info["lookups"][0] == e["first"], tag
        if "last" in e:
            assert info["lookups"][-1] == e["last"], tag
        if "ramberg" in e:
            assert info["ramberg"][0] == e["ramberg"], tag
        if e.get("snapped"):
            assert abs(abs(info["sin3"]) - 1.0) < 1.0e-12, tag
        if "rotated" in e:
            assert info["rotated"] == e["rotated"] if e["rotated"] < 2 else info["rotated"] >= e["rotated"], tag
        if "skipped" in e:
            assert info["skipped"] >= e["skipped"], tag
        if case.exit == "exhausted" and not case.apex:
            assert abs(info["residual"]) >= P.TOL ** 2 and info["iterations"] == P.MAXITER, tag
        if case.apex:
            assert not np.isfinite(s).any(), tag
        else:
            assert np.isfinite(s).all() and np.isfinite(float(fs)), tag


def test_the_exhausted_return_of_the_ramberg_deck():
    """E = 8e4, nu = 0.3, RAMBERG-OSGOOD 0.01 / 800 / 12, a uniaxial trial stress of 1500: residual 9.7e-4 after the fifth iteration"""
    case = next(c for c in P.CASES["ramberg"] if c.name == "exhausted")
    m = P.material("ramberg")
    assert (m.E, m.nu, m.harden, m.plconst) == (8.0e4, 0.3, 3, (0.01, 800.0, 12.0)) and case.stress.tolist() == [1500.0, 0, 0, 0, 0, 0]
    _, _, _, info = _run(case, np.float64)
    assert info["exit"] == "exhausted" and abs(info["residual"] - 9.7e-4) < 0.05e-4, info


@pytest.mark.parametrize("case", [c for c in P.all_cases() if c.margin], ids=["%s-%s" % (c.mat, c.name) for c in P.all_cases() if c.margin])
def test_margins_of_the_cases_beside_an_edge(case):
    kind, size = case.margin
    mat = P.material(case.mat)
    for dtype in DTYPES:
        _, _, _, info = _run(case, dtype)
        if kind == "f":
            # 0.9 tol and 1.1 tol: 1e-4 from the edge, up to the rounding of f itself (eps * 1e3 * a few operations)
            assert size == 1.0e-4 and abs(abs(info["f"]) - P.TOL) >= size - 1.0e-11, (case.name, info["f"])
        elif kind == "band":
            c, _, eta = mat.plconst
            s = case.stress
            p = (s[0] + s[1] + s[2]) / 3.0
            root = float(np.sqrt(T.mises(s) ** 2 / 3.0))
            ends = (mat.plconst4 * c - 3.0 * eta * p, mat.plconst4 * c - eta * p)
            assert size >= 1.0e-6 and min(abs(root - x) / x for x in ends) >= size, (case.name, root, ends)
            # and away from the |f| < tol band that sits on the low end
            assert abs(abs(info["f"]) - P.TOL) >= 1.0e-4 - 1.0e-11
        else:
            assert kind == "ramberg" and case.plstrain >= mat.plconst[0] * (1.0 + size)


@pytest.mark.skipif(not WIDE, reason="np.longdouble is no wider than float64 on this platform")
@pytest.mark.parametrize("name", P.MATERIAL_NAMES)
def test_float64_and_long_double_agree(name):
    """Per material, the arrays the GPU test compares: stress and (where it is written) fstat of the update cases, the tangents of
    the tangent states"""
    cases = P.CASES[name]
    a = [_run(c, np.float64) for c in cases]
    b = [_run(c, np.longdouble) for c in cases]
    smax = max(np.abs(x[0]).max() for x, c in zip(a, cases) if not c.apex)
    written = [k for k, c in enumerate(cases) if c.exit not in ("band", "elastic") and np.isfinite(float(a[k][2]))]
    fmax = max(abs(float(a[k][2])) for k in written)
    worst = [0.0, 0.0, 0.0]
    for k, c in enumerate(cases):
        assert a[k][1] == b[k][1] and a[k][3]["exit"] == b[k][3]["exit"], c.name
        fin = np.isfinite(a[k][0])
        assert np.array_equal(fin, np.isfinite(b[k][0])) and np.isfinite(float(a[k][2])) == np.isfinite(float(b[k][2])), c.name
        assert c.apex or fin.all()
        if fin.any():
            worst[0] = max(worst[0], float(np.abs(b[k][0][fin] - a[k][0][fin]).max()) / smax)
        if k in written:
            worst[1] = max(worst[1], abs(float(b[k][2] - np.longdouble(a[k][2]))) / fmax)
        elif np.isfinite(float(a[k][2])):
            assert float(b[k][2]) == float(a[k][2]) == P.SENTINEL
    mat = P.material(name)
    states = P.tangent_states()[name]
    Ds = [P.tangent(mat, st.stress, st.istat, np.float64(st.fstat)) for st in states]
    dmax = max(np.abs(D).max() for D in Ds)
    for st, D in zip(states, Ds):
        Dl = P.tangent(mat, st.stress.astype(np.longdouble), st.istat, np.longdouble(st.fstat))
        assert Dl.dtype == np.longdouble
        worst[2] = max(worst[2], float(np.abs(Dl - D).max()) / dmax)
    print("%s: %d cases, %d tangent states, float64 vs long double: stress %.1e fstat %.1e tangent %.1e" % (name, len(cases), len(states), *worst))
    assert max(worst) <= 1e-12


def test_tangent_states_take_their_branch():
    states = P.tangent_states()
    signs = set()
    for name in P.MATERIAL_NAMES:
        mat = P.material(name)
        De = Y.elastic_matrix(mat, np.dtype(np.float64))
        assert len(states[name]) >= 1
        for st in states[name]:
            for dtype in DTYPES:
                info = {}
                D = P.tangent(mat, st.stress.astype(dtype), st.istat, dtype(st.fstat), info)
                assert np.isfinite(D).all() and np.abs(D - De).max() > 1e-3 * De.max(), (name, st.name)
                if st.branch is not None:
                    assert info["branch"] == st.branch, (name, st.name, info)
                if st.sin3 is not None:
                    assert abs(info["sin3"] - st.sin3) < 1e-12, (name, st.name, info)
                    signs.add(st.sin3)
    assert signs == {-1.0, 1.0}
    edge = [st.name for st in states["multilinear"] if st.branch == "edge"]
    assert edge == ["below_first_row", "on_last_row", "beyond_last_row"]


def _exit_of_the_oracle(po, mat, case, s, ist, fs):
    """The exit the C oracle took, read off its outputs"""
    if np.array_equal(s, case.stress) and fs == case.fstat and case.fstat == P.SENTINEL:
        return "band" if ist else "elastic"
    if ist == 0:
        return "reset"
    G = mat.E / (2.0 * (1.0 + mat.nu))
    f = T.mises(case.stress) - 3.0 * G * (fs - case.plstrain) - po.curr_yield(mat, fs)
    return "converged" if abs(f) < P.TOL ** 2 else "exhausted"


@pytest.mark.parametrize("name", [k for k in P.MATERIAL_NAMES if P.family(k) == "mises"])
def test_the_mises_point_is_the_c_oracle(oracle, name):
    po = oracle
    mat = P.material(name)
    cases = P.CASES[name]
    smax = max(np.abs(P.result(c)[0]).max() for c in cases)
    fmax = max(abs(P.result(c)[2]) for c in cases if c.exit not in ("band", "elastic"))
    for c in cases:
        s, ist, fs, info = P.result(c)
        so, io, fo = po.backward_euler(mat, c.stress, c.plstrain, c.istat, c.fstat)
        assert io == ist and _exit_of_the_oracle(po, mat, c, so, io, fo) == info["exit"] == c.exit, c.name
        assert np.abs(so - s).max() <= 1e-12 * smax and abs(fo - fs) <= 1e-12 * fmax, c.name
        if c.exit in ("band", "elastic"):
            assert np.array_equal(so, c.stress) and fo == P.SENTINEL
    # the laws on their edges: every plastic strain a case or a tangent state names, and the iterates of the returns
    ps = sorted({c.plstrain for c in cases} | {P.result(c)[2] for c in cases if c.exit not in ("band", "elastic")} |
                {st.fstat for st in P.tangent_states()[name]} | (set(P.TABLE[:, 1]) if name == "multilinear" else set()))
    for p in ps:
        y, h = float(P.curr_yield(mat, np.float64(p))), float(P.harden_coeff(mat, np.float64(p)))
        assert abs(po.curr_yield(mat, p) - y) <= 1e-12 * abs(y), (name, p)
        assert abs(po.harden_coeff(mat, p) - h) <= 1e-12 * max(abs(h), 1e-300), (name, p)
    for st in P.tangent_states()[name]:
        D = P.tangent(mat, st.stress, st.istat, np.float64(st.fstat))
        assert np.abs(po.elastoplastic_matrix(mat, st.stress, st.istat, st.fstat) - D).max() <= 1e-12 * np.abs(D).max(), st.name


def test_thermal_restatement_uses_this_point():
    """nl_thermal_ref.mises_backward_euler is this module's routine"""
    import nl_thermal_ref as NT
    c = next(c for c in P.CASES["bilinear"] if c.name == "plastic")
    a = NT.mises_backward_euler(P.material("bilinear"), c.stress.astype(np.longdouble), c.plstrain, c.istat, c.fstat)
    b = c.run(np.longdouble)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[0].dtype == np.longdouble


@pytest.mark.parametrize("etype", TYPES)
def test_zero_increment_hands_over_stress_bak(oracle, etype):
    """UPDATELAG, ddu = 0: the displacement gradient is zero, so D . 0, the rotation term and vol0 add exact zeros to stress_bak.  With
    a yield surface out of reach the routines return the trial stress: array_equal to stress_bak, whatever unode is."""
    m = H.gpu_mesh(etype)
    e = 0 if etype != 361 else m.n_elem - 1          # at 361 the collapsed hexahedron
    nd = m.conn[e] - 1
    ec, nq = m.coord[nd], H.POINTS[etype]
    pool = np.array([c.stress for c in P.all_cases()])
    sb = pool[(np.arange(nq) * 5) % len(pool)]
    u = 0.01 * np.sin(3.0 * ec + 1.0)
    z = np.zeros_like(u)
    strain_bak, zq = 1.0e-3 * np.cos(np.arange(nq * 6.0)).reshape(nq, 6), np.zeros(nq)
    for un in (z, u):
        for name in ("mohr", "bilinear"):
            mat = P.out_of_reach(name)
            assert mat.nlgeom == P.UPDATELAG
            args = (ec, un, z, mat, sb, strain_bak, zq, np.zeros(nq, dtype=np.int32), zq)
            if etype == 361:
                out = Y.update_c3d8bbar(*args)
            elif name == "mohr":
                out = Y.update_c3(etype, *args)
            else:
                out = (T if etype in (341, 342) else CN).update_c3(etype, *args)
            assert np.array_equal(out[1], sb), (etype, name)
            assert np.array_equal(out[2], strain_bak) and not out[3].any()


def test_coverage_of_exits_and_principal_positions():
    exits, triples = set(), set()
    for c in P.all_cases():
        info = P.result(c)[3]
        exits.add((P.family(c.mat), info["exit"]))
        if c.mat == "mohr" and "maxp" in info:
            triples.add((info["maxp"], info["minp"], info["mm"]))
    assert exits == {("mises", "band"), ("mises", "elastic"), ("mises", "converged"), ("mises", "exhausted"),
                     ("drucker", "band"), ("drucker", "elastic"), ("drucker", "reset"), ("drucker", "converged"),
                     ("mohr", "band"), ("mohr", "elastic"), ("mohr", "converged"), ("mohr", "exhausted")}
    # the six orderings (at (1, 2) and (2, 1) the reference's rule puts mm ON the minimum / the maximum, not on the index left over),
    # and (0, 0, 1) of the all-equal apex stress
    assert triples == {(0, 2, 1), (0, 1, 2), (1, 2, 2), (1, 0, 2), (2, 1, 2), (2, 0, 1), (0, 0, 1)}
    tied = {c.expect["triple"] for c in P.CASES["mohr"] if c.name.startswith("tie_")}
    assert tied == {(0, 2, 1), (0, 1, 2), (1, 0, 2), (2, 0, 1)}
    # the tie of the issue: diag(500, 500, -900) -> (50.22, 361.36, -912.37); the last of ties would swap the first two
    s = P.result(next(c for c in P.CASES["mohr"] if c.name == "tie_hi_0"))[0]
    assert np.abs(s[:3] - [50.22, 361.36, -912.37]).max() < 0.005 and not s[3:].any()
    # the reset of the issue: mean stress 400, pure shear 161.12 -> f = 57.03, istat back to 0, the stress rebuilt from the trial one
    c = next(c for c in P.CASES["drucker"] if c.name == "reset_mid")
    s, ist, fs, info = P.result(c)
    assert abs(c.stress[3] - 161.12) < 0.01 and abs(info["f"] - 57.03) < 0.005 and ist == 0 and fs == c.plstrain
    assert np.abs(s - c.stress).max() <= 4 * EPS * np.abs(c.stress).max()


@pytest.mark.parametrize("mutant", list(P.MUTANTS))
def test_cases_tell_a_wrong_point_function_apart(mutant):
    hit = []
    for c in P.all_cases():
        if c.apex:
            continue
        s, ist, fs, _ = P.result(c)
        sm, im, fm, _ = _run(c, np.float64, **P.MUTANTS[mutant])
        moved = np.abs(sm - s).max() > 1e-9 * max(np.abs(s).max(), np.abs(sm).max())
        moved = moved or abs(float(fm) - fs) > 1e-9 * max(abs(fs), abs(float(fm)))
        if moved or im != ist:
            hit.append("%s-%s" % (c.mat, c.name))
    # a converged return does not remember the slope it started with (Newton on a piecewise linear law ends on the same root): the
    # hardening coefficient of a breakpoint shows in the tangent states
    for name, states in P.tangent_states().items():
        for st in states:
            D = P.tangent(P.material(name), st.stress, st.istat, np.float64(st.fstat))
            Dm = P.tangent(P.material(name), st.stress, st.istat, np.float64(st.fstat), **P.MUTANTS[mutant])
            if np.abs(Dm - D).max() > 1e-9 * np.abs(D).max():
                hit.append("tangent %s-%s" % (name, st.name))
    print(mutant, "->", hit)
    assert hit, "no case notices: " + mutant


@pytest.mark.parametrize("etype,nlgeom,elemopt", P.AFFINE_RUNS)
def test_affine_cells_put_every_point_in_its_branch(oracle, etype, nlgeom, elemopt):
    """The inputs of the INFINITE / TOTALLAG / F-bar comparisons (point_ref.affine_model): every point of every cell takes the branch
    of its case with the margins, and the restated update of the mesh returns what the point function alone returns there"""
    trial = P.check_affine(etype, nlgeom, elemopt)
    m, em, per_elem, st, ref = P.affine_model(etype, nlgeom, elemopt)
    ref.element_update()
    for e, c in enumerate(per_elem):
        for q, s in enumerate(trial[e]):
            out, ist, fs = P.point(P.material(c.mat, nlgeom), s, np.float64(c.plstrain), c.istat, np.float64(c.fstat))
            assert ist == ref.st["istat"][e, q] and np.abs(out - ref.st["stress"][e, q]).max() <= 1e-12 * np.abs(out).max()
            assert abs(fs - ref.st["fstat"][e, q]) <= 1e-12 * max(abs(fs), 1e-3)
            assert c.exit != "elastic" or (fs == P.SENTINEL and np.array_equal(out, s))
