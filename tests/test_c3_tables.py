"""The facts of the six solid element types -- nodes, quadrature points, getSubFace's node tables -- live once in
frontistr_amd.mesh; the names the callers and the other tests use are that object, not copies of it, and they hold what the
tests' own restatements (dload_ref, heat_ref, hyper_ref, dload_nl_decks) hold."""
import numpy as np

import dload_nl_decks as DK
import dload_ref
import heat_ref
import hyper_ref

TYPES = (341, 342, 351, 352, 361, 362)


def test_one_object_behind_every_name():
    from frontistr_amd import fstr, hecmw, mesh
    assert fstr.fstr_solid.NODES is mesh.C3_NODES and hecmw._C3_NODES is mesh.C3_NODES
    assert fstr.fstr_solid.POINTS is mesh.C3_POINTS and hecmw._C3_POINTS is mesh.C3_POINTS
    assert fstr.tDload.SUBFACE is mesh.C3_SUBFACE
    assert tuple(sorted(mesh.C3_NODES)) == tuple(sorted(mesh.C3_POINTS)) == tuple(sorted(mesh.C3_SUBFACE)) == TYPES


def test_the_tables_hold_what_the_restatements_hold():
    from frontistr_amd import mesh
    assert mesh.C3_NODES == dload_ref.NODES == heat_ref.NODES == hyper_ref.NODES
    assert mesh.C3_POINTS == hyper_ref.POINTS
    assert mesh.C3_SUBFACE == dload_ref.SUBFACE
    for et in TYPES:
        for nod in mesh.C3_SUBFACE[et]:
            assert len(set(nod)) == len(nod) and 1 <= min(nod) and max(nod) <= mesh.C3_NODES[et]
    for et, faces in DK.SUBFACE_VERTICES.items():      # the vertices of a face come first in its row
        assert tuple(nod[:len(v)] for nod, v in zip(mesh.C3_SUBFACE[et], faces)) == faces


def test_dload_faces_on_the_dload_decks():
    """the top faces of the three cantilever decks, found by the decks' own vertex table"""
    from frontistr_amd import fstr
    for name in DK.NAMES:
        et = DK.ETYPE[name]
        coord, conn = DK.cantilever(et)
        faces = fstr.dload_faces(coord, [(et, conn)], coord[:, 2] == 1.0)
        top = [(0, e, f) for e, f in DK.top_faces(et, coord, conn)]
        assert top and faces == top, (name, faces, top)     # (the mid-edge nodes of a flat top lie on the plane too)
