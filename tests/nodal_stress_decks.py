"""The decks tests/golden/make_nodal_stress_golden.py records fstr_NodalStress3D's arrays from (tests/golden/nodal_stress.npz), and
their meshes as the arrays the nodal stress pass takes.

Local node ids are positions in the !NODE card among the nodes an element names; the connectivity of TYPE=342 and 352 is brought
into fistr1's node order as hecmw2fstr_connect_conv does (heat_decks.TABLE); elements keep the file's order inside a type, the
types ascend (hecMESH%elem_type_item).  The result files list nodes and elements in that order with their global ids, which the
recording keeps and the tests compare."""
import os

import numpy as np

from heat_decks import TABLE, _cards

HERE = os.path.dirname(os.path.abspath(__file__))
DECKS = os.path.join(HERE, "golden", "decks")
GOLDEN_CNT = os.path.join(DECKS, "nodal_stress")     # the control copies the goldens were run with
# Two files, each below the size limit of a committed file: the six linear exB decks, and the two nonlinear decks
GOLDEN = os.path.join(HERE, "golden", "nodal_stress.npz")
GOLDEN_NL = os.path.join(HERE, "golden", "nodal_stress_nl.npz")

# name -> (directory under tests/golden/decks, mesh, the deck's own control file)
RECORDED = {"B%d" % t: ("static/exB", "B%d.msh" % t, "B%d.cnt" % t) for t in (341, 342, 351, 352, 361, 362)}
RECORDED["necking"] = ("t05", "necking.msh", "necking.cnt")     # NLSTATIC, Mises MULTILINEAR: the last converged sub-step (8) is recorded
# NLSTATIC, a cantilever of TYPE=361 under an end load, automatic incrementation: ten sub-steps, the last one is recorded.  It is
# here for the nodal principal vectors of a nonlinear deck: bending separates the principal stresses at every node
RECORDED["C3D8beam"] = ("autoinc", "C3D8beam.msh", "C3D8beam.cnt")
NONLINEAR = ("necking", "C3D8beam")
# linear static, 361 + 351 + 341 in one mesh (the reference's refine/hexpritet sample): nodes on the interfaces are held by elements
# of different types, so the order of addition ACROSS the groups is held against the reference itself
RECORDED["hexpritet"] = ("refine/hexpritet", "sample.msh", "sample.cnt")

# !OUTPUT_RES names -> labels of the result file (static_make_result.f90)
FIELDS = ("ISTRAIN", "ISTRESS", "NSTRAIN", "NSTRESS", "NMISES", "ESTRAIN", "ESTRESS", "EMISES", "PRINC_NSTRESS", "PRINCV_NSTRESS",
          "PRINC_NSTRAIN", "PRINC_ESTRESS", "PRINCV_ESTRESS")


def read_msh(path):
    """-> (global node ids in local order, [(etype, conn (n_elem, nn), 1-based local ids)], global element ids in hecMESH's order)"""
    ids, elems, eids = [], {}, {}
    for card, arg, v in _cards(path):
        if v is None:
            continue
        if card == "NODE":
            ids.append(int(v[0]))
        elif card == "ELEMENT":
            elems.setdefault(int(arg["TYPE"]), []).append([int(x) for x in v[1:]])
            eids.setdefault(int(arg["TYPE"]), []).append(int(v[0]))
    used = set(x for rows in elems.values() for r in rows for x in r)
    ids = [i for i in ids if i in used]
    local = {i: k + 1 for k, i in enumerate(ids)}
    groups, order = [], []
    for et in sorted(elems):
        c = np.array([[local[x] for x in r] for r in elems[et]], dtype=np.int32)
        if et in TABLE:
            c = c[:, np.array(TABLE[et]) - 1]
        groups.append((et, np.ascontiguousarray(c)))
        order += eids[et]
    return np.array(ids), groups, np.array(order)


# The rule for principal vectors: compared only where the three principal values are separated by more than 1e-6 of the largest
# magnitude, and at most 5 % of a deck's nodes or elements may be left out; a deck that is too uniform for that is replaced by
# another one, the share is not raised.  The reference alone leaves out 6.8 % of necking's NODES (the bar's axis, where two
# principal stresses coincide), so necking is not a deck of the rule for nodal vectors: C3D8beam is the nonlinear deck that is (0 %
# left out), beside the six exB decks.  necking's separated nodes are compared all the same, without a claim on their share; its
# element vectors (0.9 % left out) fall under the rule like every other deck's.
# hexpritet is a patch test: its stress is uniform and two principal values coincide everywhere, so it has no vector to compare at
# all; it is recorded for the values across groups of different types.
NODAL_VECTOR_DECKS = tuple(n for n in RECORDED if n not in ("necking", "hexpritet"))
ELEMENT_VECTOR_DECKS = tuple(n for n in RECORDED if n != "hexpritet")


def golden_file(name):
    return GOLDEN_NL if name in NONLINEAR else GOLDEN


def load(name):
    d, msh, _ = RECORDED[name]
    return read_msh(os.path.join(DECKS, d, msh))
