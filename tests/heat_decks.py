"""The reference's heat example decks (tests/golden/decks/heat/) as the arrays the heat loops take, and the list of decks that
tests/golden/make_heat_golden.py records through the unmodified fistr1 (tests/golden/heat_decks.npz).

Local node ids are the positions in the !NODE card among the nodes that an element names (HEC-MW keeps the file's order and drops
the others: the result files do not hold them); the connectivity of TYPE=342 and 352 is
brought into fistr1's node order as hecmw2fstr_connect_conv does (fistr1/src/common/hecmw2fstr_connect_conv.c, Table342 /
Table352); elements keep the file's order inside a type, the types ascend (hecMESH%elem_type_item)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DECKS = os.path.join(HERE, "golden", "decks", "heat")
GOLDEN_CNT = os.path.join(DECKS, "golden")          # the control copies (and the two transient meshes) the goldens were run with
TABLE = {342: [1, 2, 3, 4, 7, 5, 6, 8, 9, 10], 352: [1, 2, 3, 4, 5, 6, 9, 7, 8, 12, 10, 11, 13, 14, 15]}
SOLID = (341, 342, 351, 352, 361, 362)

# name -> (directory of the mesh, mesh, the deck's own control file)
RECORDED = {}
for _t in SOLID:
    RECORDED["N%d" % _t] = ("exN", "N%d.msh" % _t, "N.cnt")
    RECORDED["O%d" % _t] = ("exO", "O%d.msh" % _t, "O300.cnt")
for _m, _c in (("MA361", "A.cnt"), ("MB361", "B.cnt"), ("MG361", "G.cnt")):
    RECORDED[_m] = ("exM", _m + ".msh", _c)
# the two transient variants: their meshes (two-row density and specific heat tables, an initial temperature) and control
# files (!HEAT with fixed steps) are written by the generator into GOLDEN_CNT
RECORDED["N361T"] = ("golden", "N361T.msh", "N361T.cnt")
RECORDED["N342T"] = ("golden", "N342T.msh", "N342T.cnt")
TRANSIENT = ("N361T", "N342T")


def _cards(path):
    card, arg = None, {}
    for line in open(path):
        s = line.strip()
        if not s or s.startswith("!!") or s.startswith("#"):
            continue
        if s.startswith("!"):
            p = [x.strip() for x in s[1:].split(",")]
            card = p[0].upper().replace(" ", "")
            arg = {k.strip().upper(): v.strip() for k, v in (x.split("=", 1) for x in p[1:] if "=" in x)}
            arg["_FLAGS"] = [x.upper() for x in p[1:] if "=" not in x]
            if "=" in card:                     # `!ITEM=3, SUBITEM=1`
                k, v = card.split("=", 1)
                card, arg[k] = k, v
            yield card, arg, None
            continue
        yield card, arg, [x.strip() for x in s.split(",") if x.strip()]


def read_msh(path):
    ids, coord, local, elems, ngroups, items, init, interface, zero = [], [], {}, {}, {}, {}, [], None, 0.0
    for card, arg, v in _cards(path):
        if v is None:
            if card == "NGROUP":
                ngroups.setdefault(arg["NGRP"], [])
            continue
        if card == "NODE":
            local[int(v[0])] = len(ids) + 1
            ids.append(int(v[0]))
            coord.append([float(x) for x in v[1:4]])
        elif card == "ELEMENT":
            elems.setdefault(int(arg["TYPE"]), []).append([int(x) for x in v[1:]])
        elif card == "NGROUP":
            n = [int(x) for x in v]
            if "GENERATE" in arg["_FLAGS"]:
                n = list(range(n[0], n[1] + 1, n[2] if len(n) > 2 else 1))
            ngroups[arg["NGRP"]] += n
        elif card == "ITEM":
            items.setdefault(int(arg["ITEM"]), []).append((float(v[0]), float(v[1]) if len(v) > 1 else 0.0))
        elif card == "ZERO":
            zero = float(v[0])
        elif card == "INITIALCONDITION":
            init.append((v[0], float(v[1])))
        elif card == "SECTION" and arg.get("TYPE", "").upper() == "INTERFACE":
            interface = [float(x) for x in v]
    # nodes that no element names are not part of hecMESH (the result files do not hold them); group members among them drop out
    used = set(x for rows in elems.values() for r in rows for x in r)
    keep = [k for k, i in enumerate(ids) if i in used]
    ids, coord = [ids[k] for k in keep], [coord[k] for k in keep]
    local = {i: k + 1 for k, i in enumerate(ids)}
    ngroups = {g: [local[i] for i in n if i in local] for g, n in ngroups.items()}
    ngroups["NALL"] = list(range(1, len(ids) + 1))
    elems = {et: [[local[x] for x in r] for r in rows] for et, rows in elems.items()}
    groups = []
    for et in sorted(elems):
        c = np.array(elems[et], dtype=np.int32)
        if et in TABLE:
            c = c[:, np.array(TABLE[et]) - 1]
        groups.append((et, np.ascontiguousarray(c)))
    return dict(ids=np.array(ids), coord=np.array(coord), groups=groups, ngroups=ngroups, rho=items[1], cp=items[2], cond=items[3],
                init=init, interface=interface, zero=zero)


def read_cnt(path):
    fix, flux, heat = [], [], None
    for card, arg, v in _cards(path):
        if v is None:
            continue
        if card == "FIXTEMP":
            fix.append((v[0], float(v[1])))
        elif card == "CFLUX":
            flux.append((v[0], float(v[1])))
        elif card == "HEAT" and heat is None:
            heat = [float(x) for x in v]
    return fix, flux, heat


def load(name, cnt_dir=None):
    """the deck `name` of RECORDED with the control copy the golden was run with -> dict: coord, groups [(etype, conn, None, None)]
    of the solid types, interface (the TYPE=541 group of MG361 as (541, conn, (TZERO, THICK, HH, RR1, RR2)), or None), rows of the three tables, temp0, fix =
    (nodes, values), flux (n_node) or None, and dt, etime, dtmin, itmax, eps of the !HEAT line (dt = 0: steady)"""
    d, msh, _ = RECORDED[name]
    m = read_msh(os.path.join(DECKS, d, msh))
    fixc, fluxc, heat = read_cnt(os.path.join(GOLDEN_CNT if cnt_dir is None else cnt_dir, name + ".cnt"))
    n = m["coord"].shape[0]
    fn, fv = [], []
    for g, val in fixc:
        fn += m["ngroups"][g]
        fv += [val] * len(m["ngroups"][g])
    flux = None
    if fluxc:
        flux = np.zeros(n)
        for g, val in fluxc:
            for node in m["ngroups"][g]:
                flux[node - 1] = flux[node - 1] + val
    temp0 = np.zeros(n)
    for g, val in m["init"]:
        temp0[np.array(m["ngroups"][g]) - 1] = val
    heat = (heat or []) + [None] * 6
    dflt = (0.0, 0.0, 0.0, 0.0, 20, 1.0e-6)
    dt, etime, dtmin, _, itmax, eps = (dflt[k] if heat[k] is None else heat[k] for k in range(6))
    out = dict(m, fix=(np.array(fn, dtype=np.int32), np.array(fv)), flux=flux, temp0=temp0, dt=dt, etime=etime, dtmin=dtmin,
               itmax=int(itmax), eps=eps)
    out["interface"] = None
    out["groups"] = []
    for et, c in m["groups"]:
        if et in SOLID:
            out["groups"].append((et, c, None, None))
        elif et == 541:
            out["interface"] = (541, c, (m["zero"],) + tuple(m["interface"][:4]))     # a group heat_ref.assemble takes after the solids
        else:
            raise ValueError("element type %d" % et)
    return out


def golden(g, name):
    """(node ids, temperatures per recorded step (nstep, n_node), [[(iterALL, CHK), ...] per step]) of heat_decks.npz"""
    h = g[name + "_hist"]
    steps = [[(int(k), float(c)) for s, k, c in h if int(s) == st] for st in sorted(set(int(s) for s in h[:, 0]))]
    return g[name + "_ids"], g[name + "_temp"], steps
