"""The reference's static example decks exB..exE (tests/golden/decks/static/) for the six solid types as the arrays the distributed
load takes: mesh (numbered as nodal_stress_decks.read_msh numbers it), the FIX nodes, E, nu, the density (ITEM=2 of the mesh's
material), the !DLOAD cards of the control file resolved to (element, LTYPE, PARAMS(0:6)) entries, the solver's preconditioner and
the displacement extrema of the shipped X3nn_correct.log."""
import os
import re

import numpy as np

from heat_decks import _cards
from nodal_stress_decks import read_msh

HERE = os.path.dirname(os.path.abspath(__file__))
STATIC = os.path.join(HERE, "golden", "decks", "static")
SOLID = (341, 342, 351, 352, 361, 362)
DECKS = [(ex, t) for ex in "BCDE" for t in SOLID]
LTYPE = {"BX": 1, "BY": 2, "BZ": 3, "GRAV": 4, "CENT": 5, "P1": 10, "P2": 20, "P3": 30, "P4": 40, "P5": 50, "P6": 60}


def _groups(path, card_name, key):
    """NGROUP / EGROUP cards -> {name: [global ids]} (GENERATE rows are first, last, step)"""
    out = {}
    for card, arg, v in _cards(path):
        if card != card_name:
            continue
        name = arg[key]
        out.setdefault(name, [])
        if v is None:
            continue
        if "GENERATE" in arg["_FLAGS"]:
            out[name] += list(range(int(v[0]), int(v[1]) + 1, int(v[2]) if len(v) > 2 else 1))
        else:
            out[name] += [int(x) for x in v]
    return out


def read_log(path):
    """-> (3, 2): (max, min) of U1..U3 of the `Global Summary` block"""
    out, glob = {}, False
    for line in open(path):
        if "Global Summary" in line:
            glob = True
        m = re.match(r"\s*//(U[123])\s+([-0-9.E+]+)\s+([-0-9.E+]+)\s*$", line)
        if m and glob:
            out[m.group(1)] = (float(m.group(2)), float(m.group(3)))
    return np.array([out["U1"], out["U2"], out["U3"]])


def read_deck(ex, etype):
    d = os.path.join(STATIC, "ex" + ex)
    msh = os.path.join(d, "%s%d.msh" % (ex, etype))
    cnt = os.path.join(d, "%s%d.cnt" % (ex, etype))
    if not os.path.exists(cnt):
        cnt = os.path.join(d, "%s300.cnt" % ex)
    ids, groups, eids = read_msh(msh)
    assert len(groups) == 1 and groups[0][0] == etype
    local = {int(g): k for k, g in enumerate(ids)}                  # global node id -> 0-based local
    elocal = {int(g): k for k, g in enumerate(eids)}
    xyz, items = {}, {}
    for card, arg, v in _cards(msh):
        if v is None:
            continue
        if card == "NODE":
            xyz[int(v[0])] = [float(x) for x in v[1:4]]
        elif card == "ITEM":
            items.setdefault(int(arg["ITEM"]), [float(x) for x in v])
    coord = np.array([xyz[int(g)] for g in ids])
    ngrp, egrp = _groups(msh, "NGROUP", "NGRP"), _groups(msh, "EGROUP", "EGRP")
    egrp["ALL"] = [int(g) for g in eids]
    fix, cards, precond = [], [], 3
    for card, arg, v in _cards(cnt):
        if card == "SOLVER" and v is None:
            precond = int(arg.get("PRECOND", 3))
        if v is None:
            continue
        if card == "BOUNDARY":
            assert (int(v[1]), int(v[2]), float(v[3])) == (1, 3, 0.0)
            fix += [local[g] + 1 for g in ngrp[v[0]] if g in local]
        elif card == "DLOAD":
            par = [float(x) for x in v[2:]] + [0.0] * 7
            cards.append((np.array([elocal[g] for g in egrp[v[0]] if g in elocal]), LTYPE[v[1].upper()], par[:7]))
    fix = np.array(sorted(set(fix)), dtype=np.int32)
    log = os.path.join(d, "%s%d_correct.log" % (ex, etype))
    return dict(coord=coord, groups=[(etype, groups[0][1])], fix=fix, E=items[1][0], nu=items[1][1], rho=items.get(2, [0.0])[0],
                cards=cards, precond=precond, expect=read_log(log))


def dload_arrays(cards, group=0):
    """(group, elem, ltype, params (n, 7), None) of read_deck's cards"""
    g, e, lt, par = [], [], [], []
    for elems, ltype, p in cards:
        for el in elems:
            g.append(group); e.append(int(el)); lt.append(ltype); par.append(p)
    return (np.array(g, dtype=np.int32), np.array(e, dtype=np.int32), np.array(lt, dtype=np.int32),
            np.array(par, dtype=np.float64).reshape(-1, 7), None)
