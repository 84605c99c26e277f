"""The reference's heat example decks with surface terms (tests/golden/decks/heat/exP, exQ, exR, exS) as the arrays the heat loops
take, and the list of decks that tests/golden/make_heat_bc_golden.py records through the unmodified fistr1
(tests/golden/heat_bc_decks.npz).  Built on heat_decks.py: nodes, elements, node groups, tables, !FIXTEMP and !CFLUX are read
there; here !EGROUP, !SGROUP, !ZERO and !AMPLITUDE of the mesh file, !DFLUX / !FILM / !RADIATE (and their surface-group forms
!SDFLUX / !SFILM / !SRADIATE) with AMP, AMP1, AMP2 of the control file, and the !HEAT line with its empty fields.

A list is (group, elem, face, val[, sink], amplitude[, sink amplitude]) in the order of the reference's Q_SUF / H_SUF / R_SUF
lists: card after card, line after line, group member after group member."""
import os

import numpy as np

import heat_decks as HD

DECKS, GOLDEN_CNT, SOLID = HD.DECKS, HD.GOLDEN_CNT, HD.SOLID

# name -> (directory of the mesh, mesh, the deck's own control file)
RECORDED = {}
for _d, _c in (("P", "P%d0.cnt"), ("Q", "Q%d0.cnt"), ("R", "R%d0.cnt"), ("S", "S.cnt")):
    for _t in SOLID:
        RECORDED["%s%d" % (_d, _t)] = ("ex" + _d, "%s%d.msh" % (_d, _t), _c % (_t // 10) if "%" in _c else _c)
# two transient variants written by the generator into GOLDEN_CNT: !DFLUX (a face and BF), !FILM with an !AMPLITUDE on its sink
# and !RADIATE together, two-row density and specific heat tables, an initial temperature, the fixed steps of N361T
RECORDED["S361T"] = ("golden", "S361T.msh", "S361T.cnt")
RECORDED["S352T"] = ("golden", "S352T.msh", "S352T.cnt")
TRANSIENT = ("S361T", "S352T")
STEADY = tuple(n for n in RECORDED if n not in TRANSIENT)


def read_groups(path):
    """element ids per type in file order, !EGROUP members, !SGROUP (element, face) pairs, !AMPLITUDE rows [(value, time)]"""
    eids, egroups, sgroups, amps = {}, {}, {}, {}
    for card, arg, v in HD._cards(path):
        if v is None:
            continue
        if card == "ELEMENT":
            eids.setdefault(int(arg["TYPE"]), []).append(int(v[0]))
        elif card == "EGROUP":
            n = [int(x) for x in v]
            if "GENERATE" in arg["_FLAGS"]:
                n = list(range(n[0], n[1] + 1, n[2] if len(n) > 2 else 1))
            egroups.setdefault(arg["EGRP"], []).extend(n)
        elif card == "SGROUP":
            n = [int(x) for x in v]
            sgroups.setdefault(arg["SGRP"], []).extend(zip(n[0::2], n[1::2]))
        elif card == "AMPLITUDE":
            x = [float(t) for t in v]
            amps.setdefault(arg["NAME"], []).extend(zip(x[0::2], x[1::2]))
    return eids, egroups, sgroups, amps


def read_cnt(path):
    """[(kind, amplitude names, group, face or None for a surface group, values)] of the three cards, and the !HEAT line with its
    empty fields as None"""
    cards, heat = [], None
    for line in open(path):
        s = line.strip()
        if s.upper().replace(" ", "").startswith("!HEAT"):
            heat = []
        elif heat == [] and s and not s.startswith("!"):
            heat = [float(x) if x.strip() else None for x in s.split(",")]
        elif heat == [] and s.startswith("!") and not s.startswith("!!"):
            heat = [None]
    for card, arg, v in HD._cards(path):
        if v is None:
            continue
        kind = {"DFLUX": 0, "FILM": 1, "RADIATE": 2, "SDFLUX": 0, "SFILM": 1, "SRADIATE": 2}.get(card)
        if kind is None:
            continue
        names = (arg.get("AMP"),) if kind == 0 else (arg.get("AMP1"), arg.get("AMP2"))
        if card in ("SDFLUX", "SFILM", "SRADIATE"):
            cards.append((kind, names, v[0], None, [float(x) for x in v[1:]]))
            continue
        face = 0 if v[1].upper() == "BF" else int(v[1][1:])
        cards.append((kind, names, v[0], face, [float(x) for x in v[2:]]))
    return cards, heat


def load(name, amplitude=None, cnt_dir=None):
    """the deck `name` of RECORDED with the control copy the golden was run with -> the dict of heat_decks.load (coord, groups, the
    three tables' rows, temp0, fix, flux, dt, etime, itmax, eps, zero) plus dflux, film, radiate (lists as above, or None).
    amplitude: the class that makes an amplitude of its rows (heat_bc_ref.Amplitude, frontistr_amd.heat.tHeatAmplitude)"""
    d, msh, _ = RECORDED[name]
    path = os.path.join(DECKS, d, msh)
    cnt = os.path.join(GOLDEN_CNT if cnt_dir is None else cnt_dir, name + ".cnt")
    m = HD.read_msh(path)
    fixc, fluxc, _ = HD.read_cnt(cnt)
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
    cards, heat = read_cnt(cnt)
    heat = (heat or []) + [None] * 6
    dflt = (0.0, 0.0, 0.0, 0.0, 20, 1.0e-6)
    dt, etime, dtmin, _, itmax, eps = (dflt[k] if heat[k] is None else heat[k] for k in range(6))
    out = dict(m, fix=(np.array(fn, dtype=np.int32), np.array(fv)), flux=flux, temp0=temp0, dt=dt, etime=etime, dtmin=dtmin,
               itmax=int(itmax), eps=eps)
    out["groups"] = [(et, c, None, None) for et, c in m["groups"]]
    assert all(et in SOLID for et, _ in m["groups"])
    eids, egroups, sgroups, amps = read_groups(path)
    where = {}
    for g, et in enumerate(sorted(eids)):
        for k, e in enumerate(eids[et]):
            where[e] = (g, k)
    lists = [None, None, None]
    for kind, names, grp, face, vals in cards:
        members = [(e, face) for e in egroups[grp]] if face is not None else sgroups[grp]
        nval = 1 if kind == 0 else 2
        if lists[kind] is None:
            lists[kind] = dict(g=[], e=[], f=[], v=[[] for _ in range(nval)], names=names)
        L = lists[kind]
        assert L["names"] == names, "one amplitude per kind of card in these decks"
        for e, f in members:
            g, k = where[e]
            L["g"].append(g); L["e"].append(k); L["f"].append(f)
            for i in range(nval):
                L["v"][i].append(vals[i])
    for kind, key in enumerate(("dflux", "film", "radiate")):
        L = lists[kind]
        if L is None:
            out[key] = None
            continue
        a = tuple(None if nm is None else (amps[nm] if amplitude is None else amplitude(amps[nm])) for nm in L["names"])
        out[key] = (np.array(L["g"], dtype=np.int32), np.array(L["e"], dtype=np.int32), np.array(L["f"], dtype=np.int32)) + \
            tuple(np.array(v) for v in L["v"]) + a
    return out


def golden(g, name):
    return HD.golden(g, name)
